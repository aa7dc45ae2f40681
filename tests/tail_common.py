"""Shared by test_tail_large.py and test_gpu_tail_matrix.py: a float64 definition of the large-grid fusion tail, written
from the layer definitions alone (PixelShuffle(2) || Upsample(x2, bilinear, align_corners=True) -> cat -> Conv2d 3x3,
padding 1), and the case builders of the GPU matrix.  It shares nothing with oracle/ita_oracle.c, whose f32 fmaf chain
has the kernels' expression order: every sum here is a float64 sum, and the interpolation coordinate is the exact
rational q (T - 1) / (O - 1) rounded once to float64, not the oracle's f32 product."""
import functools

import numpy as np

from drone_oa_iree_vit_accelerator_amd import synth


def _bilinear_axis(T, O):
    """align_corners=True: output q samples the input at q (T - 1) / (O - 1) -> (i0, i1, weight of i1)"""
    q = np.arange(O, dtype=np.int64)
    src = (q * (T - 1)).astype(np.float64) / float(O - 1)
    i0 = np.minimum(np.floor(src).astype(np.int64), T - 1)
    i1 = np.minimum(i0 + 1, T - 1)
    return i0, i1, src - i0


def fused_map_f64(x, tok_h, tok_w):
    """x (B, tok_h*tok_w, E) -> the concatenated map (B, 5E/4, 2 tok_h, 2 tok_w), float64"""
    x = np.asarray(x, np.float64)
    B, T, E = x.shape
    assert T == tok_h * tok_w and E % 4 == 0
    m = x.reshape(B, tok_h, tok_w, E).transpose(0, 3, 1, 2)          # (B, E, h, w): token h*tok_w + w, channel c
    # PixelShuffle(2): out[c][2h + i][2w + j] = in[4c + 2i + j][h][w]
    ps = m.reshape(B, E // 4, 2, 2, tok_h, tok_w).transpose(0, 1, 4, 2, 5, 3).reshape(B, E // 4, 2 * tok_h, 2 * tok_w)
    y0, y1, ly = _bilinear_axis(tok_h, 2 * tok_h)
    x0, x1, lx = _bilinear_axis(tok_w, 2 * tok_w)
    rows = m[:, :, y0, :] * (1.0 - ly)[None, None, :, None] + m[:, :, y1, :] * ly[None, None, :, None]
    up = rows[:, :, :, x0] * (1.0 - lx) + rows[:, :, :, x1] * lx
    return np.concatenate([ps, up], axis=1)


def tail_f64(x, tok_h, tok_w, conv_w, conv_b):
    """the fusion tail in float64: (B, tok_h*tok_w, E), (CO, 5E/4, 3, 3), (CO,) -> (B, CO, 2 tok_h, 2 tok_w)"""
    f = fused_map_f64(x, tok_h, tok_w)
    w = np.asarray(conv_w, np.float64)
    B, CIN, OH, OW = f.shape
    assert w.shape[1:] == (CIN, 3, 3)
    pad = np.zeros((B, CIN, OH + 2, OW + 2), np.float64)
    pad[:, :, 1:-1, 1:-1] = f
    out = np.zeros((B, w.shape[0], OH, OW), np.float64) + np.asarray(conv_b, np.float64)[None, :, None, None]
    for ky in range(3):
        for kx in range(3):
            out += np.einsum("oc,bcyx->boyx", w[:, :, ky, kx], pad[:, :, ky:ky + OH, kx:kx + OW], optimize=True)
    return out


# ------------------------------------------------------------------------------------------ cases
# (E, tok_h, tok_w, out_ch): what ita_fusion_tail_large dispatches to, by its own rule -- the up kernel at E = 128,
# out_ch <= 48, tok_h % 8 == 0; else ita_tail_big_kernel<NT, 4, 3> when tok_h % 8 != 0 or NT = 4, <NT, 8, 9> otherwise.
def variant(E, th, tw, co):
    nt = (co + 15) // 16
    if E == 128 and co <= 48 and th % 8 == 0:
        return "up"
    return f"big<{nt},4,3>" if (th % 8 or nt == 4) else f"big<{nt},8,9>"


def case_id(shape):
    E, th, tw, co = shape
    return f"E{E}_{th}x{tw}_co{co}"


BIG_16ROW = [(64, 8, 16, co) for co in (16, 17, 32, 48, 49, 64)] + [(64, 24, 32, 64), (128, 8, 16, 49), (128, 8, 16, 64)]
BIG_8ROW = [(64, 4, 16, co) for co in (1, 16, 17, 32, 49, 64)] + [(E, 12, 16, co) for E in (64, 128) for co in (20, 64)]
OTHER_E = [(E, th, 16, co) for E in (16, 32, 48, 96, 256) for th in (4, 8) for co in (9, 33)]
UP = [(128, 8, 16, co) for co in (1, 9, 47)]
MATRIX = BIG_16ROW + BIG_8ROW + OTHER_E + UP
BIG = [s for s in MATRIX if variant(*s) != "up"]


@functools.lru_cache(maxsize=None)
def case(shape, B=2, seed=21):
    """seeded inputs of one matrix case, shared between tests: not to be written to"""
    E, th, tw, co = shape
    return synth.tail_large_case(seed, E, th, tw, co, B)


@functools.lru_cache(maxsize=None)
def want_f64(shape, B=2, seed=21):
    E, th, tw, co = shape
    c = case(shape, B, seed)
    out = tail_f64(c["x"], th, tw, c["conv_w"], c["conv_b"])
    out.setflags(write=False)
    return out


# one shape per kernel instantiation (the up kernel's phase 2 included), plus all_shuffle with ch > 0 (E = 256) and a
# chunk that is part shuffle, part upsample, part padding (E = 48)
EXACT = [(64, 8, 16, 16), (64, 8, 16, 17), (64, 8, 16, 48), (64, 8, 16, 64), (64, 4, 16, 1), (64, 12, 16, 20),
         (64, 4, 16, 33), (128, 12, 16, 64), (128, 8, 16, 47), (256, 8, 16, 9), (48, 4, 16, 33)]
VARIANTS = ["up"] + [f"big<{nt},{w},{t}>" for nt in (1, 2, 3) for w, t in ((8, 9), (4, 3))] + ["big<4,4,3>"]


def integer_case(shape, B=1, seed=0):
    """Integer tokens |v| <= 8, integer weights |w| <= 4 on the E/4 pixel-shuffle input channels and zero on the
    upsampled ones, integer bias: every product and partial sum is an integer far below 2^24 and every f16 lo plane
    of a value that takes part is zero, so the kernels must reproduce the float64 result exactly."""
    E, th, tw, co = shape
    rs = np.random.RandomState(977 + seed)
    w = np.zeros((co, E // 4 + E, 3, 3), np.float32)
    w[:, :E // 4] = rs.randint(-4, 5, size=(co, E // 4, 3, 3))
    w[0, 0, 0, 0] = 4.0      # the loader's power-of-two scale comes from max|w|: pin it
    return dict(x=rs.randint(-8, 9, size=(B, th * tw, E)).astype(np.float32), conv_w=w,
                conv_b=rs.randint(-16, 17, size=(co,)).astype(np.float32))
