"""Row and column statistics of the H whole S x S probability matrices of the int8 attention block with H heads, in
numpy: the definition ita_mha_long_heads_int8_stats (Engine.attention_stats_long_heads) is tested against.  Built from
mha_heads_ref's functions and nothing else, as attention_stats_ref.stats is.

Q and K are split into H runs of P / H features exactly as mha_heads_ref.mha splits them; head h's logits are
requant(Q_h . K_h^T, ML); the six statistics of attention_stats_ref.NAMES are that module's definitions applied to the
head's matrix, each (B, H, S).  At H = 1 the result is attention_stats_ref.stats with an axis of length 1 inserted.
"""
from __future__ import annotations

from typing import Dict

import numpy as np

from . import mha_heads_ref as ref
from .attention_stats_ref import NAMES


def stats_heads(x: np.ndarray, t: Dict[str, np.ndarray], H: int, l: int = 0, block: int = 512) -> Dict[str, np.ndarray]:
    """x: (B, S, E) float32 block input (or int8 codes); t: the tensors of params.attention_tensors; H: the head count;
    l: the layer.  A head's S x S matrix is formed `block` query rows at a time."""
    g = lambda k: t[f"attn{l}.{k}"]
    sc = np.asarray(g("scal"), np.float32)
    x = np.asarray(x)
    x_q = x if x.dtype == np.int8 else ref.quantize(x, sc[ref.INV_SX])
    Q = ref.split_heads(ref.linear_q(x_q, g("wq"), g("bq"), sc[ref.MQ]), H).astype(np.int32)
    Kt = ref.split_heads(ref.linear_q(x_q, g("wk"), g("bk"), sc[ref.MK]), H).astype(np.int32).transpose(0, 1, 3, 2)
    B, _, S, _ = Q.shape
    out = {k: np.zeros((B, H, S), np.int8 if k == "row_max" else np.int32) for k in NAMES}
    for r0 in range(0, S, block):
        r = slice(r0, min(r0 + block, S))
        logits = ref.requant(Q[:, :, r] @ Kt, sc[ref.ML])                       # (B, H, rows, S)
        x32 = logits.astype(np.int32)
        shift = x32.max(-1, keepdims=True) - x32
        p = ref.softmax_int(logits).astype(np.int32)
        out["row_max"][:, :, r] = logits.max(-1)
        out["row_sum"][:, :, r] = np.where(shift > 31, 0, 256 >> np.minimum(shift, 31)).sum(-1)
        out["row_mass"][:, :, r] = p.sum(-1)
        out["row_nnz"][:, :, r] = np.count_nonzero(p, axis=-1)
        out["col_mass"] += p.sum(2, dtype=np.int32)
        out["col_nnz"] += np.count_nonzero(p, axis=2).astype(np.int32)
    return out
