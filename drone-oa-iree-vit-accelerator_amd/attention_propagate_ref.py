"""Weighted column sums of the whole S x S probability matrix of the int8 attention block at H = 1, in numpy: the
definition ita_mha_long_int8_propagate (Engine.attention_propagate_long) is tested against.  Built from mha_heads_ref's
functions and nothing else.

With p = the uint8 probabilities (B, S, S) that mha_heads_ref.mha computes and int8 weights w (B, R, S):
    out[b, r, j] = sum_i w[b, r, i] * p[b, i, j]        int32 (B, R, S)
attention_stats_ref's col_mass is w = all ones, a probability row is w = one-hot.

Range: |out| <= 128 * 255 * S, and the kernel's partial sums 128 sum w + sum w (p - 128) stay inside int32 for any int8
weight at S <= 32768, and at S = 65536 for weights in [-127, 127] (127 * 128 * 65536 < 2^30 twice).
"""
from __future__ import annotations

from typing import Dict

import numpy as np

from . import mha_heads_ref as ref


def probs_rows(x: np.ndarray, t: Dict[str, np.ndarray], l: int = 0, block: int = 512):
    """yields (row slice, uint8 probabilities (B, rows, S)) of the S x S matrix, `block` query rows at a time"""
    g = lambda k: t[f"attn{l}.{k}"]
    sc = np.asarray(g("scal"), np.float32)
    x = np.asarray(x)
    x_q = x if x.dtype == np.int8 else ref.quantize(x, sc[ref.INV_SX])
    Q = ref.linear_q(x_q, g("wq"), g("bq"), sc[ref.MQ]).astype(np.int32)
    Kt = ref.linear_q(x_q, g("wk"), g("bk"), sc[ref.MK]).astype(np.int32).transpose(0, 2, 1)
    S = Q.shape[1]
    for r0 in range(0, S, block):
        r = slice(r0, min(r0 + block, S))
        yield r, ref.softmax_int(ref.requant(Q[:, r] @ Kt, sc[ref.ML]))


def propagate64(x: np.ndarray, t: Dict[str, np.ndarray], w: np.ndarray, l: int = 0, block: int = 512) -> np.ndarray:
    """the same sums for integer weights of any width, in int64: w (B, R, S) or (R, S) -> int64 (B, R, S)"""
    x = np.asarray(x)
    B, S = x.shape[0], x.shape[1]
    w = np.asarray(w)
    assert w.dtype.kind in "iu", w.dtype
    w = np.broadcast_to(w.astype(np.int64), (B,) + w.shape[-2:])
    assert w.shape[2] == S, (w.shape, S)
    out = np.zeros((B, w.shape[1], S), np.int64)
    for r, p in probs_rows(x, t, l, block):
        out += w[:, :, r] @ p.astype(np.int64)
    return out


def propagate(x: np.ndarray, t: Dict[str, np.ndarray], w: np.ndarray, l: int = 0, block: int = 512) -> np.ndarray:
    """x: (B, S, E) float32 block input (or int8 codes); t: the tensors of params.attention_tensors; w: int8 weights
    (B, R, S) or (R, S), the same for every frame; l: the layer -> int32 (B, R, S).  The S x S matrix is formed `block` query
    rows at a time; the sums are accumulated in int64 and checked to fit before the cast."""
    w = np.asarray(w)
    assert w.dtype == np.int8, w.dtype
    out = propagate64(x, t, w, l, block)
    assert np.abs(out).max(initial=0) < 2 ** 31
    return out.astype(np.int32)
