"""Per-head histograms of the H whole S x S matrices of the int8 attention block with H heads in front of and behind its
integer softmax, in numpy: the definition ita_mha_long_heads_int8_hist (Engine.attention_histograms_long_heads) is tested
against.  Built from mha_heads_ref and attention_hist_ref only.

Q and K are split into H runs of P / H features exactly as mha_heads_ref.mha splits them; head h's accumulators are
Q_h . K_h^T, and the five results of attention_hist_ref.NAMES are that module's definitions applied to the head's matrix:
logits, shifts, probs (B, H, 256) int64, logits_out (B, H, 2) int64, acc_range (B, H, 2) int32.  At H = 1 the result is
attention_hist_ref.hist with an axis of length 1 inserted.
"""
from __future__ import annotations

from typing import Dict

import numpy as np

from . import attention_hist_ref as one
from . import mha_heads_ref as ref

NAMES = one.NAMES


def _heads_qk(x, t, H, l):
    """(Q (B, H, S, P / H) float64, K^T (B, H, P / H, S) float64, ml)"""
    Q, Kt, ml = one._qk(x, t, l)
    return ref.split_heads(Q, H), ref.split_heads(Kt.transpose(0, 2, 1), H).transpose(0, 1, 3, 2), ml


def _empty(B, H):
    return {k: v.reshape(B, H, -1) for k, v in one._empty(B * H).items()}


def hist_heads(x: np.ndarray, t: Dict[str, np.ndarray], H: int, l: int = 0, block: int = 512) -> Dict[str, np.ndarray]:
    """x: (B, S, E) float32 block input (or int8 codes); t: the tensors of params.attention_tensors; H: the head count;
    l: the layer.  A head's S x S matrix is formed `block` query rows at a time."""
    Q, Kt, ml = _heads_qk(x, t, H, l)
    B, _, S, _ = Q.shape
    out = _empty(B, H)
    for r0 in range(0, S, block):
        r = slice(r0, min(r0 + block, S))
        acc = np.rint(Q[:, :, r] @ Kt).astype(np.int32)                           # (B, H, rows, S)
        raw = one._raw(acc, ml)
        logits = ref.requant(acc, ml)
        x32 = logits.astype(np.int64)
        shift = x32.max(-1, keepdims=True) - x32
        p = ref.softmax_int(logits)
        for b in range(B):
            for h in range(H):
                out["logits"][b, h] += np.bincount((x32[b, h] + 128).ravel(), minlength=256)
                out["shifts"][b, h] += np.bincount(shift[b, h].ravel(), minlength=256)
                out["probs"][b, h] += np.bincount(p[b, h].ravel(), minlength=256)
                out["logits_out"][b, h] += (np.count_nonzero(raw[b, h] < -128), np.count_nonzero(raw[b, h] > 127))
                out["acc_range"][b, h] = (min(out["acc_range"][b, h, 0], acc[b, h].min()),
                                          max(out["acc_range"][b, h, 1], acc[b, h].max()))
    return out


def hist_heads_from_classes(x_classes: np.ndarray, counts: np.ndarray, t: Dict[str, np.ndarray], H: int,
                            l: int = 0) -> Dict[str, np.ndarray]:
    """attention_hist_ref.hist_from_classes per head: the five results, (1, H, .), for ONE frame made of V distinct tokens
    x_classes (V, E) (or (1, V, E)) of which token v stands at counts[v] positions, from the H V x V matrices only."""
    x_classes = np.asarray(x_classes)
    if x_classes.ndim == 2:
        x_classes = x_classes[None]
    counts = np.asarray(counts, np.int64)
    assert x_classes.shape[0] == 1 and counts.shape == (x_classes.shape[1],) and (counts > 0).all()
    Q, Kt, ml = _heads_qk(x_classes, t, H, l)
    w = (counts[:, None] * counts[None, :]).ravel()
    weighted = lambda v: np.rint(np.bincount(v.ravel(), weights=w.astype(np.float64), minlength=256)).astype(np.int64)   # < 2^53: exact
    out = _empty(1, H)
    for h in range(H):
        acc = np.rint(Q[0, h] @ Kt[0, h]).astype(np.int32)               # (V, V): query class u, key class v
        raw = one._raw(acc, ml)
        x32 = ref.requant(acc, ml).astype(np.int64)
        shift = x32.max(-1, keepdims=True) - x32
        num = np.where(shift > 31, 0, 256 >> np.minimum(shift, 31)).astype(np.int64)
        s = np.maximum((num * counts[None, :]).sum(-1, keepdims=True), 1)      # <= 256 * 65536 = 2^24: exact in float32
        inv = np.floor((np.float32(1.0) / s.astype(np.float32)) * np.float32(16711680.0)).astype(np.int64)
        p = ((num * inv) >> 16).astype(np.uint8).astype(np.int64)
        out["logits"][0, h], out["shifts"][0, h], out["probs"][0, h] = weighted(x32 + 128), weighted(shift), weighted(p)
        out["logits_out"][0, h] = (w[(raw < -128).ravel()].sum(), w[(raw > 127).ravel()].sum())
        out["acc_range"][0, h] = (acc.min(), acc.max())
    return out
