"""Crafted conv weights and frames for the fixed 60 x 90 -> 8 x 16 tokenizer, its float64 definition and an independent
numpy model of the u8 integer conv (csrc/ita_tokenizer_kernel.h: ItaTokTab, tok_u8_tile; ita_weights_load.h: build_tok_tab).

Why: every stock E = 64 blob (synth.float_params: conv weights U(-1/7, 1/7)) has ONE exponent e_c = 24 for all channels and
synth.frames never holds pixel code 255, so the stock tests cannot tell a wrong per-channel table from a right one.

Weight sets (E = 64 and 128; bias and LayerNorm affine are the stock seed-0 ones):
    graded : channel c scaled by 2^((c % 7) - 3): seven neighbouring binades, interleaved, so adjacent channels and the
             channels of one 16-tile differ
    wide   : channel c scaled by 2^((c % 18) - 14) (weights above 1), plus DEAD (all zero), TINY (constant 2^-140: the
             scale underflows to 0), POW2 (maximum exactly a power of two), UP_POS / UP_NEG (maximum +-nextafter(0.25f, 0):
             max |w| 2^e rounds up to Wq = +-2^22)
    taps   : channel c has one non-zero weight +-(1 + c / 64) at tap c % 49
    digits : w = Wq 2^-e_c from integers Wq, e_c cycling over DIGIT_E; the first tap is +-(2^22 - 1 - c % 3) and pins the
             exponent (exactly 2^22 would move e_c by one: the edge Wq = +-2^22 needs a rounding and lives in `wide`), the
             second the other sign; every channel holds DIGIT_VALUES, where each byte plane sits at -128 and 127, both
             carries fire and w2 is at +-64

Needs numpy only (the oracle is not loaded here)."""
import functools

import numpy as np

from drone_oa_iree_vit_accelerator_amd import synth
from drone_oa_iree_vit_accelerator_amd.tokenizer_long_ref import geometry

F32 = np.float32
ES = (64, 128)
SETS = ("graded", "wide", "taps", "digits")
DEAD, TINY, POW2, UP_POS, UP_NEG = 5, 6, 7, 8, 9           # the special channels of `wide`
DIGIT_E = (21, 23, 24, 26, 28)
DIGIT_VALUES = (0x3F7F7F, -0x3F7F7F, 0x3F7F80, -0x3F7F80, 0x3F8080, -0x3F8080, 0x7F7F, -0x7F7F, 0x8080, -0x8080,
                0x80, -0x80, 0x8000, -0x8000, 0x7F, -0x7F, 0x7F80, -0x7F80, 0)
BOUND = 1e-5       # the project's bound of a tokenizer definition against float64 (tests/test_tokenizer_long_cpu.py)


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def stock(E):
    """(cw (E, 49), cb, ln_w, ln_b) of synth.float_params(0, E)"""
    fp = synth.float_params(0, E=E)
    return _ro(np.ascontiguousarray(fp["tokenizer.conv.weight"].reshape(E, 49)), fp["tokenizer.conv.bias"].copy(),
               fp["tokenizer.norm.weight"].copy(), fp["tokenizer.norm.bias"].copy())


def digit_integers(E):
    """(Wq (E, 49) int64, e (E,) int64) of the `digits` set"""
    rs = np.random.RandomState(7700 + E)
    wq = rs.randint(-(1 << 22) + 8, (1 << 22) - 7, size=(E, 49)).astype(np.int64)
    e = np.array([DIGIT_E[c % len(DIGIT_E)] for c in range(E)], np.int64)
    for c in range(E):
        sign = 1 if c % 2 == 0 else -1
        wq[c, 0] = sign * ((1 << 22) - 1 - c % 3)
        wq[c, 1] = -sign * ((1 << 22) - 1 - (c + 1) % 3)
        wq[c, 2 + rs.permutation(47)[:len(DIGIT_VALUES)]] = DIGIT_VALUES
    return wq, e


@functools.lru_cache(maxsize=None)
def weights(E, name):
    """(cw (E, 49), cb, ln_w, ln_b) float32, read-only"""
    cw0, cb, lw, lb = stock(E)
    c = np.arange(E)
    if name == "stock":
        cw = cw0.copy()
    elif name == "graded":
        cw = cw0 * np.ldexp(F32(1), (c % 7) - 3).astype(F32)[:, None]
    elif name == "wide":
        cw = cw0 * np.ldexp(F32(1), (c % 18) - 14).astype(F32)[:, None]
        cw[DEAD] = 0
        cw[TINY] = np.ldexp(F32(1), -140)
        cw[POW2, 3] = np.ldexp(F32(1), -9)                 # the channel's other weights are below 2^-7 / 7
        assert np.abs(cw[POW2]).max() == cw[POW2, 3]
        up = np.nextafter(F32(0.25), F32(0))
        cw[UP_POS], cw[UP_NEG] = cw0[UP_POS], cw0[UP_NEG]  # stock weights: all below 1/7
        cw[UP_POS, 10], cw[UP_NEG, 40] = up, -up
    elif name == "taps":
        cw = np.zeros((E, 49), F32)
        cw[c, c % 49] = np.where(c % 2 == 0, 1, -1).astype(F32) * (F32(1) + c.astype(F32) / F32(64))
    elif name == "digits":
        wq, e = digit_integers(E)
        cw = np.ldexp(wq.astype(np.float64), -e[:, None]).astype(F32)
        assert np.array_equal(np.ldexp(cw.astype(np.float64), e[:, None]), wq)   # exactly the integers times 2^-e_c
    else:
        raise KeyError(name)
    assert cw.dtype == F32 and cw.shape == (E, 49) and np.isfinite(cw).all()
    return _ro(cw, cb, lw, lb)


ONE_HOT = ((0, 0), (0, 89), (59, 0), (59, 89), (30, 87), (30, 88), (30, 89), (31, 0), (31, 1), (31, 2))
FRAME_NAMES = ("zeros", "full", "checker", "uniform", "extremes") + tuple(f"hot_{r}_{c}" for r, c in ONE_HOT)
ZEROS, FULL = 0, 1
FIRST_HOT = 5
# frame byte r * 90 + c of a one-hot pixel is also the byte at (r2, c2) outside the frame: window columns 0..2 of the next
# row (image columns -3..-1) and 93..95 of the previous one (90..92), which the window masks to zero
ALIASES = {(0, 89): ((1, -1),), (30, 87): ((31, -3),), (30, 88): ((31, -2),), (30, 89): ((31, -1),),
           (59, 0): ((58, 90),), (31, 0): ((30, 90),), (31, 1): ((30, 91),), (31, 2): ((30, 92),)}


@functools.lru_cache(maxsize=None)
def frames():
    """(len(FRAME_NAMES), 60, 90) uint8, read-only"""
    rs = np.random.RandomState(7800)
    f = np.zeros((len(FRAME_NAMES), 60, 90), np.uint8)
    f[1] = 255
    yy, xx = np.mgrid[0:60, 0:90]
    f[2] = np.where((yy + xx) % 2 == 0, 0, 255)
    f[3] = rs.randint(0, 256, size=(60, 90))
    f[4] = np.array([0, 1, 254, 255], np.uint8)[rs.randint(0, 4, size=(60, 90))]
    for i, (r, c) in enumerate(ONE_HOT):
        f[FIRST_HOT + i, r, c] = 255
    return _ro(f)[0]


def frames_f32(u8):
    """the f32 form of u8 frames as the reference host makes it: float(code) / 255.0f"""
    return np.asarray(u8).astype(F32) / F32(255)


# ---------------------------------------------------------------------------------------------- geometry
def _geo():
    (y0, yp, ly), (x0, xp, lx) = geometry(60, 90, 8, 16)
    assert yp.all() and xp.all()                           # the second neighbour is always one conv row / column on
    return y0, ly, x0, lx


def reads(r, c):
    """(128,) bool: tokens of which one of the four blended 7 x 7 patches covers the position (r, c) -- also a position
    outside the frame, where the patch reads the zero border"""
    y0, _, x0, _ = _geo()
    ry, rx = r - (2 * y0 - 3), c - (2 * x0 - 3)            # patch rows 0..6 (first neighbour), 2..8 (second)
    return (((ry >= 0) & (ry <= 8))[:, None] & ((rx >= 0) & (rx <= 8))[None, :]).reshape(128)


def footprint(r, c):
    """(128,) bool: the tokens whose two-by-two blended 7 x 7 patches contain pixel (r, c)"""
    assert 0 <= r < 60 and 0 <= c < 90
    return reads(r, c)


def _neighbours(u8):
    """the four neighbours' pixel codes of every tap: four (B, 8, 16, 49) int64 arrays a, b, c, d"""
    u8 = np.asarray(u8).reshape(-1, 60, 90)
    y0, _, x0, _ = _geo()
    pad = np.zeros((u8.shape[0], 68, 98), np.int64)
    pad[:, 3:63, 3:93] = u8
    ky, kx = np.divmod(np.arange(49), 7)
    ra = (2 * y0)[:, None, None] + ky[None, None, :]       # padded row of pixel row 2 y0 - 3 + ky
    ca = (2 * x0)[None, :, None] + kx[None, None, :]
    return pad[:, ra, ca], pad[:, ra, ca + 2], pad[:, ra + 2, ca], pad[:, ra + 2, ca + 2]


def blended_taps(u8):
    """B256 (B, 128, 49) int64: 256 * 255 * the blended patch value, an exact integer (H = 8 h, W = 32 w)"""
    _, ly, _, lx = _geo()
    H1, W1 = (8 * ly.astype(np.float64)), (32 * lx.astype(np.float64))
    assert (H1 == np.rint(H1)).all() and (W1 == np.rint(W1)).all()
    H1, W1 = H1.astype(np.int64)[None, :, None, None], W1.astype(np.int64)[None, None, :, None]
    assert ((0 < H1) & (H1 < 8)).all() and ((0 < W1) & (W1 < 32)).all()
    a, b, c, d = _neighbours(u8)
    t = (8 - H1) * ((32 - W1) * a + W1 * b) + H1 * ((32 - W1) * c + W1 * d)
    return t.reshape(t.shape[0], 128, 49)


def tokens_f64(u8, cw, cb, lw, lb):
    """the tokenizer in float64 from the exact pixel values code / 255: (B, 128, E) float64"""
    _, ly, _, lx = _geo()
    h1, w1 = ly.astype(np.float64)[None, :, None, None], lx.astype(np.float64)[None, None, :, None]
    a, b, c, d = (v.astype(np.float64) / 255.0 for v in _neighbours(u8))
    pb = (1.0 - h1) * ((1.0 - w1) * a + w1 * b) + h1 * ((1.0 - w1) * c + w1 * d)
    pre = pb.reshape(pb.shape[0], 128, 49) @ np.asarray(cw, np.float64).T + np.asarray(cb, np.float64)
    mean = pre.mean(-1, keepdims=True)
    var = ((pre - mean) ** 2).mean(-1, keepdims=True)
    return (pre - mean) / np.sqrt(var + 1e-5) * np.asarray(lw, np.float64) + np.asarray(lb, np.float64)


@functools.lru_cache(maxsize=None)
def tokens_f64_of(E, name):
    """tokens_f64 of every frame on a weight set, computed once, read-only"""
    return _ro(tokens_f64(frames(), *weights(E, name)))[0]


# ---------------------------------------------------------------------------------------------- the integer conv
def quantise(cw):
    """(Wq (E, 49) int64, e (E,) int64, s (E,) float32): Wq = rne(w 2^e), e = 22 - exponent(max |w|) (0 for an all-zero
    channel), s = 2^-e / 65280 in float32"""
    cw = np.asarray(cw, F32)
    mx = np.abs(cw).max(axis=1)
    _, ex = np.frexp(mx)                                   # mx = m 2^ex, m in [0.5, 1)
    e = np.where(mx > 0, 22 - ex.astype(np.int64), 0)
    wq = np.rint(np.ldexp(cw.astype(np.float64), e[:, None])).astype(np.int64)   # exact product, one rounding to even
    s = np.ldexp(np.ones(len(e), F32), -e.astype(np.int32)) / F32(65280)
    assert s.dtype == F32
    return wq, e, s


def byte_planes(wq, carry=True):
    """Wq = 65536 w2 + 256 w1 + w0 with balanced digits w0, w1 in [-128, 127].  carry=False: the low bytes read as signed
    without handing their carry on (a mutation)"""
    wq = np.asarray(wq, np.int64)
    w0 = ((wq + 128) & 255) - 128
    r1 = (wq - w0) >> 8 if carry else wq >> 8
    w1 = ((r1 + 128) & 255) - 128
    w2 = (r1 - w1) >> 8 if carry else r1 >> 8
    return w0, w1, w2


def fma32(a, b, c):
    """float32 fma(a, b, c) with ONE rounding: the product of two float32 is exact in float64; the float64 sum is made
    round-to-odd from its exact error (TwoSum), which a final rounding to float32 (29 bits shorter) cannot see"""
    p = np.asarray(a, F32).astype(np.float64) * np.asarray(b, F32).astype(np.float64)
    c = np.broadcast_to(np.asarray(c, F32).astype(np.float64), p.shape)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    other = np.nextafter(s, np.where(err > 0, np.inf, -np.inf))
    even = (s.view(np.int64) & 1) == 0
    return np.where((err != 0) & even, other, s).astype(F32)


def _i32(x):
    assert (np.abs(x) < (1 << 31)).all()
    return x.astype(np.int32)


def tok_u8_model(u8, cw, cb, swap_scale=False, i2_without_w1=False, no_carry=False):
    """pre-LayerNorm conv output (B, 128, E) float32 of the u8 tokenizer as the kernel and its table compute it: byte planes,
    pixels' bytes as signed a ^ 0x80, the corrections in the accumulators' initial values, six int32 sums, two float32 fmas.
    Mutations: swap_scale (channel c takes the scales of channel c ^ 1), i2_without_w1 (I2 lacks its sum of w1),
    no_carry (unbalanced digits)"""
    wq, _, s = quantise(cw)
    w0, w1, w2 = byte_planes(wq, carry=not no_carry)
    assert all((w >= -128).all() and (w <= 127).all() for w in (w0, w1, w2))      # they are int8 in the table
    i0 = _i32(128 * w0.sum(1) + 32768 * (w1.sum(1) + w0.sum(1)))
    i2 = _i32(128 * (w2.sum(1) + (0 if i2_without_w1 else w1.sum(1))) + 32768 * w2.sum(1))
    s16 = F32(65536) * s
    if swap_scale:
        s, s16 = s[np.arange(len(s)) ^ 1], s16[np.arange(len(s)) ^ 1]
    t = blended_taps(u8)
    assert t.min() >= 0 and t.max() <= 65280
    a0 = ((t & 255) ^ 0x80).astype(np.uint8).view(np.int8).astype(np.int64)       # = a0 - 128
    a1 = ((t >> 8) ^ 0x80).astype(np.uint8).view(np.int8).astype(np.int64)
    mm = lambda a, w: _i32(a @ w.T)                                               # one int8 MFMA chain: (B, 128, E)
    s0 = i0.astype(np.int64) + mm(a0, w0)
    s1 = mm(a1, w0).astype(np.int64) + mm(a0, w1)
    s2 = i2.astype(np.int64) + mm(a1, w1) + mm(a0, w2)
    s3 = mm(a1, w2)
    lo = _i32(_i32(s0) + (_i32(s1).astype(np.int64) << 8))
    hi = _i32(_i32(s2) + (s3.astype(np.int64) << 8))
    return fma32(hi.astype(F32), s16, fma32(lo.astype(F32), s, np.asarray(cb, F32)))
