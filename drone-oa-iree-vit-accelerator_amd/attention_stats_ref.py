"""Row and column statistics of the whole S x S probability matrix of the int8 attention block at H = 1, in numpy: the
definition ita_mha_long_int8_stats (Engine.attention_stats_long) is tested against.  Built from mha_heads_ref's
functions and nothing else.

With p = the uint8 probabilities (B, S, S) that mha_heads_ref.mha computes:
    row_max  (B, S) int8    the row maximum of the int8 logits
    row_sum  (B, S) int32   sum_j 256 >> min(max - logit, 31), 0 beyond 31: what the probabilities are divided by
    row_mass (B, S) int32   sum_j p[i, j]      256 if the integer softmax lost nothing, 0 for a row it killed
    row_nnz  (B, S) int32   #{j : p[i, j] > 0}
    col_mass (B, S) int32   sum_i p[i, j]      "attention received" by key j
    col_nnz  (B, S) int32   #{i : p[i, j] > 0}
"""
from __future__ import annotations

from typing import Dict

import numpy as np

from . import mha_heads_ref as ref

NAMES = ("row_max", "row_sum", "row_mass", "row_nnz", "col_mass", "col_nnz")


def stats(x: np.ndarray, t: Dict[str, np.ndarray], l: int = 0, block: int = 512) -> Dict[str, np.ndarray]:
    """x: (B, S, E) float32 block input (or int8 codes); t: the tensors of params.attention_tensors; l: the layer.
    The S x S matrix is formed `block` query rows at a time."""
    g = lambda k: t[f"attn{l}.{k}"]
    sc = np.asarray(g("scal"), np.float32)
    x = np.asarray(x)
    x_q = x if x.dtype == np.int8 else ref.quantize(x, sc[ref.INV_SX])
    Q = ref.linear_q(x_q, g("wq"), g("bq"), sc[ref.MQ]).astype(np.int32)
    Kt = ref.linear_q(x_q, g("wk"), g("bk"), sc[ref.MK]).astype(np.int32).transpose(0, 2, 1)
    B, S, _ = Q.shape
    out = {k: np.zeros((B, S), np.int8 if k == "row_max" else np.int32) for k in NAMES}
    for r0 in range(0, S, block):
        r = slice(r0, min(r0 + block, S))
        logits = ref.requant(Q[:, r] @ Kt, sc[ref.ML])
        x32 = logits.astype(np.int32)
        shift = x32.max(-1, keepdims=True) - x32
        p = ref.softmax_int(logits).astype(np.int32)
        out["row_max"][:, r] = logits.max(-1)
        out["row_sum"][:, r] = np.where(shift > 31, 0, 256 >> np.minimum(shift, 31)).sum(-1)
        out["row_mass"][:, r] = p.sum(-1)
        out["row_nnz"][:, r] = np.count_nonzero(p, axis=-1)
        out["col_mass"] += p.sum(1, dtype=np.int32)
        out["col_nnz"] += np.count_nonzero(p, axis=1).astype(np.int32)
    return out


def stats_from_row(y: np.ndarray, S: int) -> Dict[str, np.ndarray]:
    """the closed form for ONE frame whose S queries all share the probability row y (S uint8): row_mass, row_nnz,
    col_mass, col_nnz, each (S,) int32"""
    y = np.asarray(y).astype(np.int32)
    assert y.shape == (S,)
    return dict(row_mass=np.full(S, y.sum(), np.int32), row_nnz=np.full(S, np.count_nonzero(y), np.int32),
                col_mass=(S * y).astype(np.int32), col_nnz=(S * (y > 0)).astype(np.int32))
