"""Weighted column sums of the H whole S x S probability matrices of the int8 attention block with H heads, in numpy:
the definition ita_mha_long_heads_int8_propagate (Engine.attention_propagate_long_heads) is tested against.  Built from
mha_heads_ref's functions and nothing else, as attention_stats_heads_ref.stats_heads is.

Q and K are split into H runs of P / H features exactly as mha_heads_ref.mha splits them; with p_hd = the uint8
probabilities of head hd and int8 weights w (B, R, S), shared by the heads:
    out[b, hd, r, j] = sum_i w[b, r, i] * p_hd[b, i, j]        int32 (B, H, R, S)
attention_stats_heads_ref's col_mass is w = all ones, a probability row of a head is w = one-hot.  At H = 1 the result is
attention_propagate_ref.propagate with an axis of length 1 inserted; its range statement holds per head.
"""
from __future__ import annotations

from typing import Dict

import numpy as np

from . import mha_heads_ref as ref


def propagate_heads64(x: np.ndarray, t: Dict[str, np.ndarray], w: np.ndarray, H: int, l: int = 0, block: int = 512) -> np.ndarray:
    """the sums for integer weights of any width, in int64: w (B, R, S) or (R, S) -> int64 (B, H, R, S).  A head's S x S
    matrix is formed `block` query rows at a time."""
    g = lambda k: t[f"attn{l}.{k}"]
    sc = np.asarray(g("scal"), np.float32)
    x = np.asarray(x)
    x_q = x if x.dtype == np.int8 else ref.quantize(x, sc[ref.INV_SX])
    Q = ref.split_heads(ref.linear_q(x_q, g("wq"), g("bq"), sc[ref.MQ]), H).astype(np.int32)
    Kt = ref.split_heads(ref.linear_q(x_q, g("wk"), g("bk"), sc[ref.MK]), H).astype(np.int32).transpose(0, 1, 3, 2)
    B, _, S, _ = Q.shape
    w = np.asarray(w)
    assert w.dtype.kind in "iu", w.dtype
    w = np.broadcast_to(w.astype(np.int64), (B,) + w.shape[-2:])
    assert w.shape[2] == S, (w.shape, S)
    out = np.zeros((B, H, w.shape[1], S), np.int64)
    for r0 in range(0, S, block):
        r = slice(r0, min(r0 + block, S))
        p = ref.softmax_int(ref.requant(Q[:, :, r] @ Kt, sc[ref.ML]))          # (B, H, rows, S)
        out += w[:, None, :, r] @ p.astype(np.int64)
    return out


def propagate_heads(x: np.ndarray, t: Dict[str, np.ndarray], w: np.ndarray, H: int, l: int = 0, block: int = 512) -> np.ndarray:
    """x: (B, S, E) float32 block input (or int8 codes); t: the tensors of params.attention_tensors; w: int8 weights
    (B, R, S) or (R, S), the same for every frame; H: the head count; l: the layer -> int32 (B, H, R, S).  The sums are
    accumulated in int64 and checked to fit before the cast."""
    w = np.asarray(w)
    assert w.dtype == np.int8, w.dtype
    out = propagate_heads64(x, t, w, H, l, block)
    assert np.abs(out).max(initial=0) < 2 ** 31
    return out.astype(np.int32)
