"""The int8 attention block with H heads, in numpy: the definition the multi-head kernel is tested against.

ITASelfAttention_QAT.forward (reference models/ITA/QAT/layers.py:101-127) splits Q, K and V into H heads of P / H
features, runs matmul1 -> integer softmax -> matmul2 per head, and concatenates the contexts.  ``matmul1`` and ``matmul2``
are one QFunctional each, so ALL heads share one logit multiplier and one context multiplier.  Everything is exact:

* accumulation in int32;
* the four Linear layers and matmul1: ``clip(rint(f32(acc + bias_q) * f32(m)), -128, 127)``;
* matmul2: the same with the ``mc`` multiplier, on the uint8 probabilities;
* the integer softmax of models/ITA/QAT/ITA_softmax.py:51-61 over the 128 keys of one head.

With H = 1 this is the block the C oracle computes (tests/test_heads_cpu.py holds the two equal); the C oracle has one
head only.  Nothing here imports it.
"""
from __future__ import annotations

from typing import Dict, Tuple

import numpy as np

f32 = np.float32
# indices of attn{i}.scal (include/ita_weights.h, params.attention_tensors)
INV_SX, MQ, MK, MV, ML, MC, MO, SO = range(8)


def requant(acc: np.ndarray, mult) -> np.ndarray:
    """int32 accumulators -> int8 codes: clip(rint(f32(acc) * f32(mult)), -128, 127)"""
    return np.clip(np.rint(acc.astype(np.float32) * f32(mult)), -128, 127).astype(np.int8)


def quantize(x: np.ndarray, inv_scale) -> np.ndarray:
    """QuantStub: clip(rint(x * (1 / s)), -128, 127)"""
    return np.clip(np.rint(np.asarray(x, np.float32) * f32(inv_scale)), -128, 127).astype(np.int8)


def linear_q(x_q: np.ndarray, w: np.ndarray, bias_q: np.ndarray, mult) -> np.ndarray:
    """nnq.Linear: x_q (..., K) int8, w (N, K) int8, bias_q (N,) int32 in accumulator units -> (..., N) int8"""
    acc = x_q.astype(np.int32) @ w.astype(np.int32).T + bias_q.astype(np.int32)
    return requant(acc, mult)


def softmax_int(logits: np.ndarray) -> np.ndarray:
    """the integer softmax over the last axis: int8 logits -> uint8 probabilities"""
    x = logits.astype(np.int32)
    shift = x.max(-1, keepdims=True) - x                    # 0 .. 255
    num = np.where(shift > 31, 0, 256 >> np.minimum(shift, 31)).astype(np.int32)
    s = np.maximum(num.sum(-1, keepdims=True), 1)
    # torch evaluates int / int32 tensor as reciprocal(tensor) * int in float32, then floor
    inv = np.floor((f32(1.0) / s.astype(np.float32)) * f32(16711680.0)).astype(np.int32)
    return ((num * inv) >> 16).astype(np.uint8)


def split_heads(a: np.ndarray, H: int) -> np.ndarray:
    """(B, S, P) -> (B, H, S, P / H): head h holds features [h P/H, (h+1) P/H)"""
    B, S, P = a.shape
    return a.reshape(B, S, H, P // H).transpose(0, 2, 1, 3)


def logits_from(Q: np.ndarray, K: np.ndarray, H: int, ml) -> Tuple[np.ndarray, np.ndarray]:
    """matmul1 per head -> (int8 logits (B, H, S, S), their int32 accumulators)"""
    acc = split_heads(Q, H).astype(np.int32) @ split_heads(K, H).astype(np.int32).transpose(0, 1, 3, 2)
    return requant(acc, ml), acc


def ctx_from(probs: np.ndarray, V: np.ndarray, H: int, mc) -> np.ndarray:
    """matmul2 per head, heads concatenated: probs (B, H, S, S) uint8, V (B, S, P) int8 -> (B, S, P) int8"""
    B, S, P = V.shape
    acc = probs.astype(np.int32) @ split_heads(V, H).astype(np.int32)       # (B, H, S, P / H)
    return requant(acc, mc).transpose(0, 2, 1, 3).reshape(B, S, P)


def mha(x: np.ndarray, t: Dict[str, np.ndarray], H: int = 1, i: int = 0):
    """x: (B, S, E) float32 block input, or int8 codes x_q; t: the blob-name keyed tensors of params.attention_tensors.
    Returns (out (B, S, E) float32, taps): x_q, Q, K, V, ctx, out_q int8; logits int8 and probs uint8, both
    (B, H, S, S), or (B, S, S) at H = 1 as the engine returns them."""
    g = lambda k: t[f"attn{i}.{k}"]
    sc = np.asarray(g("scal"), np.float32)
    P = g("wq").shape[0]
    if H < 1 or P % H:
        raise ValueError(f"H = {H} does not divide P = {P}")
    x = np.asarray(x)
    x_q = x if x.dtype == np.int8 else quantize(x, sc[INV_SX])
    Q = linear_q(x_q, g("wq"), g("bq"), sc[MQ])
    K = linear_q(x_q, g("wk"), g("bk"), sc[MK])
    V = linear_q(x_q, g("wv"), g("bv"), sc[MV])
    logits, _ = logits_from(Q, K, H, sc[ML])
    probs = softmax_int(logits)
    ctx = ctx_from(probs, V, H, sc[MC])
    out_q = linear_q(ctx, g("wo"), g("bo"), sc[MO])
    out = out_q.astype(np.float32) * sc[SO]
    if H == 1:
        logits, probs = logits[:, 0], probs[:, 0]
    return out, dict(x_q=x_q, Q=Q, K=K, V=V, logits=logits, probs=probs, ctx=ctx, out_q=out_q)
