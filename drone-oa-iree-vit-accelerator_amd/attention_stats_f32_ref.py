"""Row and column statistics of the whole S x S softmax matrix of the float attention block (one head, no 1 / sqrt(d)), in
numpy: what ita_mha_long_f32_stats (Engine.attention_stats_long_f32) is tested against.

    row_max  (B, S) f32     the row maximum m of the logits s = Q K^T
    row_sum  (B, S) f32     l = sum_j e^(s - m)
    row_gap  (B, S) f32     sum_j p (m - s) >= 0;  row_entropy = log(row_sum) + row_gap
    row_nnz  (B, S) int32   #{j : p[i, j] >= p_min}
    col_mass (B, S) f32     sum_i p[i, j]       "attention received" by key j; a frame's masses add up to S
    col_nnz  (B, S) int32   #{i : p[i, j] >= p_min}

stats64 is the definition in float64 from the parameters.  stats_from_taps is the definition applied to the kernels' own
f32 logits, row maxima and row sums (Engine.mha_long_f32_taps, all rows): the f32 probabilities
p = ita_expf(logits - row_max) * (1 / row_sum) as the library forms them, exact counts, and sums taken in float64 over
those f32 values -- the GPU's fixed-order f32 sums are held to these within the bound of any f32 sum of n terms.
"""
from __future__ import annotations

from typing import Dict

import numpy as np

NAMES = ("row_max", "row_sum", "row_gap", "row_nnz", "col_mass", "col_nnz")
P_MIN = 1.0 / 256


def gamma(n: int) -> float:
    """n u / (1 - n u), u = 2^-24: the relative error bound of an f32 sum of n non-negative terms in any fixed order"""
    u = 2.0 ** -24
    return n * u / (1.0 - n * u)


def stats64(x: np.ndarray, fp: Dict[str, np.ndarray], layer: int = 0, p_min: float = P_MIN) -> Dict[str, np.ndarray]:
    """x: (B, S, E) tokens; fp: the float parameters (attention_blocks.<layer>.{q,k}_proj.{weight,bias}).  Everything in
    float64, counts int32; besides NAMES the dict holds row_entropy"""
    g = lambda k: np.asarray(fp[f"attention_blocks.{layer}.{k}"], np.float64)
    x = np.asarray(x, np.float64)
    q = x @ g("q_proj.weight").T + g("q_proj.bias")
    k = x @ g("k_proj.weight").T + g("k_proj.bias")
    s = q @ k.transpose(0, 2, 1)
    m = s.max(-1)
    e = np.exp(s - m[..., None])
    l = e.sum(-1)
    p = e / l[..., None]
    out = _reduce(p, m[..., None] - s, p_min)
    out.update(row_max=m, row_sum=l)
    out["row_entropy"] = np.log(l) + out["row_gap"]
    return out


def _reduce(p, d, p_min):
    """p, d = m - s: (B, S, S) -> row_gap, row_nnz, col_mass, col_nnz; the sums in float64"""
    p64 = p.astype(np.float64)
    keep = p >= p.dtype.type(p_min)
    return dict(row_gap=(p64 * d.astype(np.float64)).sum(-1), row_nnz=keep.sum(-1).astype(np.int32),
                col_mass=p64.sum(-2), col_nnz=keep.sum(-2).astype(np.int32))


def expf(a: np.ndarray) -> np.ndarray:
    """ita_expf over an f32 array through the oracle's scalar (oracle.lib().ita_oracle_expf).  Its first operation clamps
    the argument to [-87, 88], so everything at or below -87 shares one call."""
    from oracle import oracle
    f = oracle.lib().ita_oracle_expf
    a = np.ascontiguousarray(a, np.float32)
    out = np.full(a.shape, f(-87.0), np.float32)
    live = a > np.float32(-87.0)
    out[live] = np.fromiter((f(float(v)) for v in a[live]), np.float32, int(live.sum()))
    return out


def probs_f32(logits: np.ndarray, row_max: np.ndarray, row_sum: np.ndarray) -> np.ndarray:
    """the library's f32 probability: one subtraction, ita_expf, one division, one multiplication, each rounded to f32"""
    logits, row_max, row_sum = (np.asarray(v, np.float32) for v in (logits, row_max, row_sum))
    return expf(logits - row_max[..., None]) * (np.float32(1.0) / row_sum)[..., None]


def stats_from_taps(logits: np.ndarray, row_max: np.ndarray, row_sum: np.ndarray, p_min: float = P_MIN) -> Dict[str, np.ndarray]:
    """logits (B, S, S), row_max, row_sum (B, S): the f32 taps of ALL rows.  -> NAMES, row_entropy and probs: the f32
    probabilities (B, S, S); row_max and row_sum are passed through, counts are exact, sums are float64 sums of the f32
    probabilities and of the float64 products p (m - s) of the f32 values"""
    logits, row_max, row_sum = (np.asarray(v, np.float32) for v in (logits, row_max, row_sum))
    p = probs_f32(logits, row_max, row_sum)
    out = _reduce(p, row_max.astype(np.float64)[..., None] - logits.astype(np.float64), np.float32(p_min))
    out.update(row_max=row_max, row_sum=row_sum, probs=p)
    out["row_entropy"] = np.log(row_sum.astype(np.float64)) + out["row_gap"]
    return out
