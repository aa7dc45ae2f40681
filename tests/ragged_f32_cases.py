"""The ragged long FLOAT attention tests' case table, inputs and references (CPU only; everything cached is read-only).
Valid tokens: long_f32_common.ln_like rows times linspace(0.5, 1.5, len) (the ramp: a row's maximum keeps moving to later
64-key units, so the masked last unit rescales) or its reverse; padding rows: seeded noise at 4 x that amplitude
(test_long_f32_ragged_cpu.py holds the inputs to what that must achieve).  References per frame, on x[b, :len_b] alone:
float64 (attn64 / layer64) and e_torch, the error of torch's CPU f32 result on the same rows (long_f32_common.bound)."""
import functools

import numpy as np

import long_f32_common as lc

# (S_pad, lens).  Units of 64 keys: nu = 1 masked (1, 63) and full (64), nu = 2 masked (65, 127); several query tiles: nu = 3
# masked (129) and unmasked (192: odd nu), nu = 4 (200), nu = 5 (257: the K ring wraps twice); a mixed batch
CASES = [(128, (1,)), (128, (63,)), (128, (64,)), (128, (65,)), (128, (127,)), (256, (129,)), (256, (192,)), (256, (200,)),
         (384, (257,)), (384, (384, 129, 1, 0, 256, 320))]
case_id = lambda c: f"{c[0]}-{'_'.join(map(str, c[1]))}"


@functools.lru_cache(maxsize=None)
def inputs(E, S_pad, lens, rev=False):
    """x (B, S_pad, E) f32"""
    rs = np.random.RandomState(11 + S_pad + sum(lens) + E)
    x = (4.0 * rs.standard_normal((len(lens), S_pad, E))).astype(np.float32)
    for b, n in enumerate(lens):
        ramp = np.linspace(0.5, 1.5, n, dtype=np.float32)
        x[b, :n] = lc.ln_like(1, n, E, 7 * S_pad + b + E)[0] * (ramp[::-1] if rev else ramp)[:, None]
    x.setflags(write=False)
    return x


def _attn_torch(twin, x, layer):
    import torch
    with torch.no_grad():
        return twin._attention(torch.from_numpy(x.copy()), layer).numpy()


@functools.lru_cache(maxsize=None)
def refs(what, E, S_pad, lens, rev=False, layer=0):
    """what = "attn" | "layer" -> per frame (float64 result on x[b, :len_b], e_torch); the empty frame: no rows, 0"""
    f64, f32 = (lc.attn64, _attn_torch) if what == "attn" else (lc.layer64, lc.layer_torch)
    fp, _, twin = lc.case(E)
    x, out = inputs(E, S_pad, lens, rev), []
    for b, n in enumerate(lens):
        want = f64(x[b:b + 1, :n], fp, layer)[0] if n else np.zeros((0, E))
        out.append((want, float(np.abs(f32(twin, x[b:b + 1, :n], layer)[0] - want).max()) if n else 0.0))
    return out
