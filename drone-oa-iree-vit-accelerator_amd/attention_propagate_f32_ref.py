"""Weighted column sums of the whole S x S softmax matrix of the float attention block (one head, no 1 / sqrt(d)), in
numpy: what ita_mha_long_f32_propagate (Engine.attention_propagate_long_f32) is tested against.

    out[b, r, j] = sum_i w[b, r, i] * p[b, i, j]          w (B, R, S), or (R, S) for every frame

propagate64 is the definition in float64 from the parameters.  propagate_from_taps is the definition applied to the
kernels' own f32 probabilities of ALL rows (Engine.attention_rows_long_f32): float64 sums of the float64 products of the
f32 values, and beside them sum_i |w| p, which the bound of a fixed-order f32 sum needs:

    |out_f32 - sum_i w p| <= gamma_(S+2) * sum_i |w| p,      gamma_n = n u / (1 - n u),  u = 2^-24

(S terms in any fixed order, one rounding for a product, one to spare).
"""
from __future__ import annotations

from typing import Dict, Tuple

import numpy as np


def gamma(n: int) -> float:
    """n u / (1 - n u), u = 2^-24"""
    u = 2.0 ** -24
    return n * u / (1.0 - n * u)


def _weights(w: np.ndarray, B: int, S: int) -> np.ndarray:
    w = np.asarray(w, np.float64)
    if w.ndim == 2:
        w = np.broadcast_to(w[None], (B,) + w.shape)
    if w.ndim != 3 or w.shape[0] != B or w.shape[2] != S:
        raise ValueError(f"w must be ({B}, R, {S}) or (R, {S}), got {w.shape}")
    return w


def probs64(x: np.ndarray, fp: Dict[str, np.ndarray], layer: int, r0: int, r1: int) -> np.ndarray:
    """rows r0 .. r1 - 1 of softmax(Q K^T) in float64: (B, r1 - r0, S)"""
    g = lambda k: np.asarray(fp[f"attention_blocks.{layer}.{k}"], np.float64)
    x = np.asarray(x, np.float64)
    q = x[:, r0:r1] @ g("q_proj.weight").T + g("q_proj.bias")
    k = x @ g("k_proj.weight").T + g("k_proj.bias")
    s = q @ k.transpose(0, 2, 1)
    e = np.exp(s - s.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def propagate64(x: np.ndarray, fp: Dict[str, np.ndarray], w: np.ndarray, layer: int = 0, block: int = 1024) -> np.ndarray:
    """x: (B, S, E) tokens; fp: the float parameters; w: (B, R, S) or (R, S) -> float64 (B, R, S).  The matrix is formed
    `block` query rows at a time and the blocks are added in order"""
    B, S = x.shape[0], x.shape[1]
    w = _weights(w, B, S)
    out = np.zeros(w.shape, np.float64)
    for r0 in range(0, S, block):
        r1 = min(r0 + block, S)
        out += w[:, :, r0:r1] @ probs64(x, fp, layer, r0, r1)
    return out


def propagate_from_taps(probs: np.ndarray, w: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """probs: (B, S, S) f32, the taps' probabilities of all rows; w: (B, R, S) or (R, S), f32 values ->
    (sum_i w p, sum_i |w| p), float64 (B, R, S) each"""
    p = np.asarray(probs, np.float32).astype(np.float64)
    w = _weights(np.asarray(w, np.float32), p.shape[0], p.shape[1])
    return w @ p, np.abs(w) @ p
