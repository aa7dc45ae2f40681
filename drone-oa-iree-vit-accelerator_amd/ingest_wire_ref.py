"""Definition of the wire ingest (ita_ingest_wire / Engine.ingest_wire): (N,H,W) u8 camera frames -> (N,60,90) u8 wire
frames with the resize the reference HOST applies before it feeds the graph (samples/inference_trainingset_custom_dispatch/
main.cpp:117-128: stbir_resize_uint8_linear to 90 x 60, one channel).  In the vendored stb_image_resize2 "linear" names
the colour space; the filter is the library's default, Mitchell (B = C = 1/3) where an axis shrinks and Catmull-Rom
where it grows or keeps its size, edge mode clamp.  numpy only, no torch.

This file restates that resize from its formulas:
  resize_tables(n_in, n_out)       per axis: first source index, tap count and normalised f32 weights of every output
  ingest_wire_reference(frames)    pixel = f32(code) * 3.9215689e-03f; vertical pass, then horizontal, taps ascending from
                                   an accumulator of 0.0f, every multiply and add rounded to float32 by itself (no fma);
                                   code = trunc(clamp(y * 255.0f + 0.5f, 0, 255))

The HIP kernel (csrc/ita_ingest_wire_kernel.h) and the C++ table builder (ita_resize_table) equal this file bit for bit.
stb itself sums its taps in another (SIMD) order, so its codes differ from these where y * 255 + 0.5 lies within rounding of
an integer: tests/test_ingest_wire_cpu.py holds this file to stb's own output (tests/golden/resize_stb_*.npz): every code
within 1, and a differing code only at such a tie.
"""
import math

import numpy as np

OUT_H, OUT_W = 60, 90
MAX_DIM = 4096
F = np.float32
U8_TO_UNIT = F(3.9215689e-03)          # stb multiplies by the rounded inverse of 255, it does not divide
SMALL = F(2.0 ** -120)                 # weights below this are taken as zero


def _mitchell(x):
    x = F(abs(x))
    if x < F(1):
        return (F(16) + x * x * (F(21) * x - F(36))) / F(18)
    if x < F(2):
        return (F(32) + x * (F(-60) + x * (F(36) - F(7) * x))) / F(18)
    return F(0)


def _catmull_rom(x):
    x = F(abs(x))
    if x < F(1):
        return F(1) - x * x * (F(2.5) - F(1.5) * x)
    if x < F(2):
        return F(2) - x * (F(4) + x * (F(0.5) * x - F(2.5)))
    return F(0)


def _floor(v):
    return int(math.floor(float(v)))


def _raw_taps(n_in, n_out):
    """per output pixel (first index, [f32 weights]) before normalisation; indices may lie outside [0, n_in)"""
    scale = F(n_out) / F(n_in)
    inv = F(n_in) / F(n_out)
    first = [0] * n_out
    taps = [[] for _ in range(n_out)]
    if scale < F(1):
        # every input pixel, from a margin in front of the row to a margin behind it, scatters onto the outputs in reach
        radius = F(2) * inv
        margin = int(math.ceil(float(F(4) / scale))) // 2
        for i in range(-margin, n_in + margin):
            centre = F(i) + F(0.5)
            oc = centre * scale
            lo = max(_floor((centre - radius) * scale + F(0.5)), 0)
            hi = min(_floor((centre + radius) * scale - F(0.5)), n_out - 1)
            for o in range(lo, hi + 1):
                c = _mitchell((F(o) + F(0.5)) - oc) * scale
                if -SMALL < c < SMALL:
                    c = F(0)
                if not taps[o] or (len(taps[o]) == 1 and taps[o][0] == F(0)):    # a zero in front is dropped
                    first[o], taps[o] = i, [c]
                else:
                    taps[o] += [F(0)] * (i - first[o] - len(taps[o])) + [c]
    else:
        radius = F(2) * scale
        for o in range(n_out):
            c = F(o) + F(0.5)
            centre = c * inv
            lo = _floor((c - radius) * inv + F(0.5))
            hi = max(_floor((c + radius) * inv - F(0.5)), lo)
            hi = min(hi, lo + 3)                                   # four taps at the most
            first[o] = lo
            for p in range(lo, hi + 1):
                w = _catmull_rom(centre - (F(p) + F(0.5)))
                if -SMALL < w < SMALL:
                    if not taps[o]:
                        first[o] = p + 1                           # zeros in front are dropped
                        continue
                    w = F(0)
                taps[o].append(w)
            while taps[o] and taps[o][-1] == F(0):
                taps[o].pop()
    return first, taps


def _normalise(n0, w):
    """weights / their sum: the sum and the division in double, the quotient rounded to f32"""
    if not w:
        raise ValueError("an output pixel without taps")
    total = 0.0
    for c in w:
        total += float(c)
    if -float(SMALL) < total < float(SMALL):
        n0, w = n0, [F(0)]
    elif total != 1.0:
        k = 1.0 / total
        w = [F(float(c) * k) for c in w]
    return n0, w


def _clamp(n_in, n0, w):
    """indices outside [0, n_in) folded onto the edge pixel by f32 addition; zeros at the end dropped"""
    w = list(w)
    n1 = n0 + len(w) - 1
    if n1 > n_in - 1:                                              # behind the end first, ascending
        for i in range(n_in, n1 + 1):
            w[n_in - 1 - n0] = w[n_in - 1 - n0] + w[i - n0]
        w = w[:n_in - n0]
    if n0 < 0:                                                     # then in front, from -1 downwards
        for i in range(-1, n0, -1):
            w[-n0] = w[-n0] + w[i - n0]
        head = w[0]
        w = w[-n0:]
        w[0] = w[0] + head
        n0 = 0
    while len(w) > 1 and w[-1] == F(0):
        w.pop()
    return n0, w


_TABLES = {}


def resize_tables(n_in, n_out):
    """one axis: n0[n_out] int32, count[n_out] int32, coeff[n_out, width] f32 (zero padded): output o is
    sum_j coeff[o, j] * source[n0[o] + j], j < count[o], every source index inside [0, n_in)"""
    key = (int(n_in), int(n_out))
    if key not in _TABLES:
        if not (1 <= key[0] <= MAX_DIM and key[1] >= 1):
            raise ValueError(f"n_in must be in [1, {MAX_DIM}] and n_out positive, got {key}")
        first, taps = _raw_taps(*key)
        # n_out / n_in = num / den in lowest terms: the weights repeat every num outputs, den source pixels further on.
        # stb computes the first num outputs only and copies the rest, so do we (the positions of the later outputs
        # round differently in f32, and their weights would differ in the last bit)
        g = math.gcd(*key)
        num, den = key[1] // g, key[0] // g
        rows = [_normalise(f, t) for f, t in zip(first[:num], taps[:num])]
        for o in range(num, key[1]):
            rows.append((rows[o - num][0] + den, rows[o - num][1]))
        rows = [_clamp(key[0], f, t) for f, t in rows]
        width = max(len(w) for _, w in rows)
        n0 = np.array([f for f, _ in rows], np.int32)
        count = np.array([len(w) for _, w in rows], np.int32)
        coeff = np.zeros((key[1], width), np.float32)
        for o, (_, w) in enumerate(rows):
            coeff[o, :len(w)] = w
        assert (n0 >= 0).all() and (n0 + count <= key[0]).all()
        _TABLES[key] = (n0, count, coeff)
    return _TABLES[key]


def ingest_wire_reference(frames_u8, return_values=False):
    """(..., H, W) uint8 -> (N, 60, 90) uint8; with return_values also y * 255 + 0.5 (f32, before clamp and truncation)"""
    a = np.asarray(frames_u8)
    if a.dtype != np.uint8:
        raise TypeError(f"frames must be uint8, got {a.dtype}")
    if a.ndim < 2:
        raise ValueError(f"frames must be (..., H, W), got {a.shape}")
    H, W = a.shape[-2:]
    if not (1 <= H <= MAX_DIM and 1 <= W <= MAX_DIM):
        raise ValueError(f"H and W must be in [1, {MAX_DIM}], got {H} x {W}")
    a = a.reshape(-1, H, W)
    px = a.astype(np.float32) * U8_TO_UNIT
    n0y, cy, wy = resize_tables(H, OUT_H)
    n0x, cx, wx = resize_tables(W, OUT_W)
    t = np.empty((a.shape[0], OUT_H, W), np.float32)
    for oy in range(OUT_H):
        acc = np.zeros((a.shape[0], W), np.float32)
        for i in range(cy[oy]):
            acc = acc + wy[oy, i] * px[:, n0y[oy] + i, :]
        t[:, oy] = acc
    y = np.empty((a.shape[0], OUT_H, OUT_W), np.float32)
    for ox in range(OUT_W):
        acc = np.zeros((a.shape[0], OUT_H), np.float32)
        for j in range(cx[ox]):
            acc = acc + wx[ox, j] * t[:, :, n0x[ox] + j]
        y[:, :, ox] = acc
    v = y * F(255) + F(0.5)
    codes = np.clip(v, F(0), F(255)).astype(np.uint8)
    return (codes, v) if return_values else codes
