"""Histograms of the whole S x S matrix of the int8 attention block at H = 1 in front of and behind its integer softmax, in
numpy: the definition ita_mha_long_int8_hist (Engine.attention_histograms_long) is tested against.  Built from
mha_heads_ref's functions and nothing else.

With acc = the int32 Q K^T accumulators (no bias term), raw = rint(f32(acc) * f32(ml)), logits = clip(raw, -128, 127) and
p = softmax_int(logits), per frame:
    logits     (B, 256) int64   bin c + 128 = #{(i, j) : logits[i, j] = c}
    logits_out (B, 2)   int64   #{raw < -128}, #{raw > 127}: what the clamp changed
    acc_range  (B, 2)   int32   minimum and maximum of acc
    shifts     (B, 256) int64   bin s = #{(i, j) : max_j' logits[i, j'] - logits[i, j] = s}
    probs      (B, 256) int64   bin v = #{(i, j) : p[i, j] = v}
"""
from __future__ import annotations

from typing import Dict

import numpy as np

from . import mha_heads_ref as ref

NAMES = ("logits", "logits_out", "acc_range", "shifts", "probs")


def _qk(x, t, l):
    """(Q (B, S, P) float64, K^T (B, P, S) float64, ml): the codes are small integers, so float64 products are exact"""
    g = lambda k: t[f"attn{l}.{k}"]
    sc = np.asarray(g("scal"), np.float32)
    x = np.asarray(x)
    x_q = x if x.dtype == np.int8 else ref.quantize(x, sc[ref.INV_SX])
    Q = ref.linear_q(x_q, g("wq"), g("bq"), sc[ref.MQ]).astype(np.float64)
    Kt = ref.linear_q(x_q, g("wk"), g("bk"), sc[ref.MK]).astype(np.float64).transpose(0, 2, 1)
    return Q, Kt, sc[ref.ML]


def _raw(acc, ml):
    """the rounded logits in front of the clamp, int64; ref.requant is clip(this, -128, 127)"""
    return np.rint(acc.astype(np.float32) * np.float32(ml)).astype(np.int64)


def _empty(B):
    out = {k: np.zeros((B, 256), np.int64) for k in ("logits", "shifts", "probs")}
    out["logits_out"] = np.zeros((B, 2), np.int64)
    out["acc_range"] = np.stack([np.full(B, np.iinfo(np.int32).max, np.int32), np.full(B, np.iinfo(np.int32).min, np.int32)], axis=1)
    return {k: out[k] for k in NAMES}


def hist(x: np.ndarray, t: Dict[str, np.ndarray], l: int = 0, block: int = 512) -> Dict[str, np.ndarray]:
    """x: (B, S, E) float32 block input (or int8 codes); t: the tensors of params.attention_tensors; l: the layer.
    The S x S matrix is formed `block` query rows at a time (the product in float64: exact, |acc| <= 192 * 128 * 128)."""
    Q, Kt, ml = _qk(x, t, l)
    B, S, _ = Q.shape
    out = _empty(B)
    for r0 in range(0, S, block):
        r = slice(r0, min(r0 + block, S))
        acc = np.rint(Q[:, r] @ Kt).astype(np.int32)
        raw = _raw(acc, ml)
        logits = ref.requant(acc, ml)
        x32 = logits.astype(np.int64)
        shift = x32.max(-1, keepdims=True) - x32
        p = ref.softmax_int(logits)
        for b in range(B):
            out["logits"][b] += np.bincount((x32[b] + 128).ravel(), minlength=256)
            out["shifts"][b] += np.bincount(shift[b].ravel(), minlength=256)
            out["probs"][b] += np.bincount(p[b].ravel(), minlength=256)
            out["logits_out"][b] += (np.count_nonzero(raw[b] < -128), np.count_nonzero(raw[b] > 127))
            out["acc_range"][b] = (min(out["acc_range"][b, 0], acc[b].min()), max(out["acc_range"][b, 1], acc[b].max()))
    return out


def hist_from_classes(x_classes: np.ndarray, counts: np.ndarray, t: Dict[str, np.ndarray], l: int = 0) -> Dict[str, np.ndarray]:
    """The same five results, each with a leading axis of 1, for ONE frame made of V distinct tokens x_classes (V, E) (or
    (1, V, E)) of which token v stands at counts[v] positions, from the V x V matrix only: the row maximum is taken over
    the classes, the row sum is sum_v counts[v] * (256 >> shift), every bin is weighted by counts[u] * counts[v]."""
    x_classes = np.asarray(x_classes)
    if x_classes.ndim == 2:
        x_classes = x_classes[None]
    counts = np.asarray(counts, np.int64)
    assert x_classes.shape[0] == 1 and counts.shape == (x_classes.shape[1],) and (counts > 0).all()
    Q, Kt, ml = _qk(x_classes, t, l)
    acc = np.rint(Q[0] @ Kt[0]).astype(np.int32)                     # (V, V): query class u, key class v
    raw = _raw(acc, ml)
    x32 = ref.requant(acc, ml).astype(np.int64)
    shift = x32.max(-1, keepdims=True) - x32
    num = np.where(shift > 31, 0, 256 >> np.minimum(shift, 31)).astype(np.int64)
    s = np.maximum((num * counts[None, :]).sum(-1, keepdims=True), 1)          # <= 256 * 65536 = 2^24: exact in float32
    inv = np.floor((np.float32(1.0) / s.astype(np.float32)) * np.float32(16711680.0)).astype(np.int64)
    p = ((num * inv) >> 16).astype(np.uint8).astype(np.int64)
    w = (counts[:, None] * counts[None, :]).ravel()
    weighted = lambda v: np.rint(np.bincount(v.ravel(), weights=w.astype(np.float64), minlength=256)).astype(np.int64)   # < 2^53: exact
    out = _empty(1)
    out["logits"][0], out["shifts"][0], out["probs"][0] = weighted(x32 + 128), weighted(shift), weighted(p)
    out["logits_out"][0] = (w[(raw < -128).ravel()].sum(), w[(raw > 127).ravel()].sum())
    out["acc_range"][0] = (acc.min(), acc.max())
    return out
