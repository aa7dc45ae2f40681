"""Definition of the ingest stage: refine_inputs' resize of camera-resolution depth frames to 60 x 90 (reference
models/ITA_single_layer_upsample_shuffle/QAT/model.py:29-30, F.interpolate(..., mode='bilinear', align_corners=False)),
restated in numpy with every operation a separately rounded float32 operation (no fused multiply-add).  The HIP kernel
(csrc/ita_ingest_kernel.h) equals this function bit for bit; it is the DEFINITION, torch's own kernels round their
weights differently (tests/test_ingest_cpu.py measures by how much).

ATen's area_pixel_compute_source_index / guard_index_and_lambda, per axis (n source pixels, m = 60 or 90 outputs):

    scale   = f32(n) / f32(m)                                     one IEEE division
    real(d) = max(scale * (f32(d) + 0.5f) - 0.5f, 0)
    i0      = min(floor(real), n - 1)      i1 = min(i0 + 1, n - 1)
    l1      = real - f32(i0)               l0 = 1 - l1
    out[y][x] = hy0 * (wx0 * a + wx1 * b) + hy1 * (wx0 * c + wx1 * d)     a, b = row y0 at x0, x1;  c, d = row y1

Pixel value before blending:
    uint8     f32(code) / 255.0f, correctly rounded (the reference hosts' float(pixel) / 255.0f, main.cpp:118,125)
    uint16    min(f32(code) * depth_scale, 1.0f)
    float32   taken as is

Needs numpy only.
"""
import numpy as np

OUT_H, OUT_W = 60, 90
MAX_DIM = 4096
DEFAULT_DEPTH_SCALE = 1.0 / 65535.0

_F = np.float32


def axis_table(n: int, m: int):
    """(i0, i1, l0, l1) of the m output positions over n source pixels: int64 indices, float32 weights"""
    scale = _F(n) / _F(m)
    d = np.arange(m, dtype=_F)
    real = np.maximum(scale * (d + _F(0.5)) - _F(0.5), _F(0))
    i0 = np.minimum(np.floor(real).astype(np.int64), n - 1)
    i1 = np.minimum(i0 + 1, n - 1)
    l1 = real - i0.astype(_F)
    l0 = _F(1) - l1
    assert real.dtype == _F and l1.dtype == _F and l0.dtype == _F
    return i0, i1, l0, l1


def pixel_values(frames: np.ndarray, depth_scale: float = DEFAULT_DEPTH_SCALE) -> np.ndarray:
    """the float32 value of every pixel before blending"""
    if frames.dtype == np.uint8:
        return frames.astype(_F) / _F(255.0)
    if frames.dtype in (np.uint16, np.int16):
        return np.minimum(frames.view(np.uint16).astype(_F) * _F(depth_scale), _F(1.0))
    if frames.dtype == _F:
        return frames
    raise TypeError(f"ingest_reference takes uint8, uint16, int16 (as the same bits) or float32 frames, got {frames.dtype}")


def ingest_reference(frames, depth_scale: float = DEFAULT_DEPTH_SCALE) -> np.ndarray:
    """frames (..., H, W) uint8 / uint16 / float32, H and W in [1, 4096] -> (N, 60, 90) float32"""
    frames = np.asarray(frames)
    if frames.ndim < 2:
        raise ValueError(f"frames must be (..., H, W), got shape {frames.shape}")
    H, W = frames.shape[-2:]
    if not (1 <= H <= MAX_DIM and 1 <= W <= MAX_DIM):
        raise ValueError(f"H and W must be in [1, {MAX_DIM}], got {H} x {W}")
    v = pixel_values(np.ascontiguousarray(frames).reshape(-1, H, W), depth_scale)
    y0, y1, hy0, hy1 = axis_table(H, OUT_H)
    x0, x1, wx0, wx1 = axis_table(W, OUT_W)
    r0, r1 = v[:, y0, :], v[:, y1, :]
    top = wx0 * r0[:, :, x0] + wx1 * r0[:, :, x1]
    bot = wx0 * r1[:, :, x0] + wx1 * r1[:, :, x1]
    out = hy0[None, :, None] * top + hy1[None, :, None] * bot
    assert out.dtype == _F
    return out
