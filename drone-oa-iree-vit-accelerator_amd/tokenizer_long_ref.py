"""Definition of the long-sequence tokenizer: the reference's OverlapPatchMerging(in, out, 7, 2, 3, output_size)
(models/ITA/QAT/layers.py:39-45: conv 7x7 stride 2 padding 3, F.interpolate(..., mode='bilinear', align_corners=False) to
the token grid, LayerNorm) for any frame size H x W and any token grid tok_h x tok_w, restated in numpy with every
operation a separately rounded float32 operation.  The HIP kernel (csrc/ita_tokenizer_long_kernel.h) equals it bit for bit.

Conv and resize are both linear, so the four bilinear neighbours are blended on the 7 x 7 INPUT patches first and the conv
runs once per token -- the order of the project's fixed 60 x 90 -> 8 x 16 tokenizer (oracle/ita_oracle.c:
ita_oracle_blend_patch), which this module generalises:

    conv grid   CH = (H - 1) // 2 + 1,  CW = (W - 1) // 2 + 1
    per axis    scale = f32(in) / f32(out),  src = max(scale * (f32(dst) + 0.5f) - 0.5f, 0)          in = CH / CW,
                i0 = min(int(src), in - 1),  ip = 1 if i0 < in - 1 else 0,  l1 = src - f32(i0)        out = tok_h / tok_w
    tap (ky, kx) of token (oy, ox):   pb[ky * 7 + kx] = h0 * (w0 * a + w1 * b) + h1 * (w0 * c + w1 * d)
                a, b = pixels (2 y0 - 3 + ky, 2 x0 - 3 + kx [+ 2 xp]),  c, d = the same in row + 2 yp,  0 outside the frame
                h1 = ly, h0 = 1 - ly, w1 = lx, w0 = 1 - lx
    token       LayerNorm(conv_b[c] + sum_k pb[k] * conv_w[c][k]): one ascending-k fmaf chain started from the bias, then
                the project's LayerNorm (sums in four blocks of E / 4 channels); row oy * tok_w + ox of the frame

Pixel value before blending: ingest_ref.pixel_values (u8 code / 255.0f, u16 min(code * depth_scale, 1.0f), f32 as is).

blend_patches gives the (B, tok_h * tok_w, 49) blended patches; the fmaf chain and the LayerNorm are the test oracle's
linear_f32 and add_ln (this module does not load the oracle).  tokens_f64 evaluates the same map in float64.

Needs numpy only.
"""
import numpy as np

from .ingest_ref import DEFAULT_DEPTH_SCALE, MAX_DIM, pixel_values

_F = np.float32

__all__ = ["geometry", "pixel_values", "blend_patches", "tokens_f64", "conv_grid"]


def conv_grid(height: int, width: int):
    """output size of the 7 x 7, stride 2, padding 3 convolution"""
    return (height - 1) // 2 + 1, (width - 1) // 2 + 1


def _axis(n_in: int, n_out: int):
    """the oracle's bilinear_src for every dst of one axis: (i0 int64, ip int64, l1 float32)"""
    scale = _F(n_in) / _F(n_out)
    dst = np.arange(n_out, dtype=_F)
    src = np.maximum(scale * (dst + _F(0.5)) - _F(0.5), _F(0))
    i0 = np.minimum(src.astype(np.int64), n_in - 1)      # src >= 0: the truncation is floor
    ip = (i0 < n_in - 1).astype(np.int64)
    l1 = src - i0.astype(_F)
    assert src.dtype == _F and l1.dtype == _F
    return i0, ip, l1


def geometry(height: int, width: int, tok_h: int, tok_w: int):
    """((y0, yp, ly), (x0, xp, lx)): source row / column on the conv grid, whether a second neighbour exists, and its
    weight, for every token row and every token column"""
    if not (1 <= height <= MAX_DIM and 1 <= width <= MAX_DIM):
        raise ValueError(f"height and width must be in [1, {MAX_DIM}], got {height} x {width}")
    if tok_h < 1 or tok_w < 1:
        raise ValueError(f"token grid must be positive, got {tok_h} x {tok_w}")
    CH, CW = conv_grid(height, width)
    return _axis(CH, tok_h), _axis(CW, tok_w)


def _frames(frames, depth_scale):
    frames = np.asarray(frames)
    if frames.ndim < 2:
        raise ValueError(f"frames must be (..., H, W), got shape {frames.shape}")
    H, W = frames.shape[-2:]
    v = pixel_values(np.ascontiguousarray(frames).reshape(-1, H, W), DEFAULT_DEPTH_SCALE if depth_scale is None else depth_scale)
    return v, H, W


def blend_patches(frames, tok_h: int, tok_w: int, depth_scale=None) -> np.ndarray:
    """frames (..., H, W) uint8 / uint16 / int16 / float32 -> (B, tok_h * tok_w, 49) float32 blended 7 x 7 patches"""
    v, H, W = _frames(frames, depth_scale)
    (y0, yp, ly), (x0, xp, lx) = geometry(H, W, tok_h, tok_w)
    B = v.shape[0]
    # zero border: 3 in front (the padding), 3 + 2 behind (the padding and the second neighbour's reach past an even size)
    pad = np.zeros((B, H + 8, W + 8), _F)
    pad[:, 3:3 + H, 3:3 + W] = v
    h1, w1 = ly[:, None], lx[None, :]
    h0, w0 = _F(1) - h1, _F(1) - w1
    out = np.empty((B, tok_h, tok_w, 49), _F)
    for ky in range(7):
        ra = (2 * y0 + ky)[:, None]                     # padded row of pixel row 2 y0 - 3 + ky
        rc = (2 * y0 + ky + 2 * yp)[:, None]
        for kx in range(7):
            ca = (2 * x0 + kx)[None, :]
            cb = (2 * x0 + kx + 2 * xp)[None, :]
            a, b, c, d = pad[:, ra, ca], pad[:, ra, cb], pad[:, rc, ca], pad[:, rc, cb]
            t = h0 * (w0 * a + w1 * b) + h1 * (w0 * c + w1 * d)
            assert t.dtype == _F
            out[..., ky * 7 + kx] = t
    return out.reshape(B, tok_h * tok_w, 49)


def tokens_f64(frames, tok_h: int, tok_w: int, conv_w, conv_b, ln_w, ln_b, depth_scale=None) -> np.ndarray:
    """the same map evaluated in float64 from the float32 pixel values and geometry: (B, tok_h * tok_w, E) float64"""
    v, H, W = _frames(frames, depth_scale)
    (y0, yp, ly), (x0, xp, lx) = geometry(H, W, tok_h, tok_w)
    B = v.shape[0]
    pad = np.zeros((B, H + 8, W + 8), np.float64)
    pad[:, 3:3 + H, 3:3 + W] = v
    h1, w1 = ly.astype(np.float64)[:, None], lx.astype(np.float64)[None, :]
    h0, w0 = 1.0 - h1, 1.0 - w1
    pb = np.empty((B, tok_h, tok_w, 49), np.float64)
    for ky in range(7):
        ra, rc = (2 * y0 + ky)[:, None], (2 * y0 + ky + 2 * yp)[:, None]
        for kx in range(7):
            ca, cb = (2 * x0 + kx)[None, :], (2 * x0 + kx + 2 * xp)[None, :]
            pb[..., ky * 7 + kx] = h0 * (w0 * pad[:, ra, ca] + w1 * pad[:, ra, cb]) + h1 * (w0 * pad[:, rc, ca] + w1 * pad[:, rc, cb])
    cw = np.asarray(conv_w, np.float64)
    E = cw.shape[0]
    pre = pb.reshape(B, tok_h * tok_w, 49) @ cw.reshape(E, 49).T + np.asarray(conv_b, np.float64)
    mean = pre.mean(-1, keepdims=True)
    var = ((pre - mean) ** 2).mean(-1, keepdims=True)
    return (pre - mean) / np.sqrt(var + 1e-5) * np.asarray(ln_w, np.float64) + np.asarray(ln_b, np.float64)
