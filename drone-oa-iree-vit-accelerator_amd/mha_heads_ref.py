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

``ffn`` is the FFN block in the same style, and both return, on request, the int32 accumulators in front of every
requantisation (tests/test_requant_cpu.py holds them to the C oracle; tests/requant_common.py crafts blobs on them).
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


def linear_acc(x_q: np.ndarray, w: np.ndarray, bias_q: np.ndarray) -> np.ndarray:
    """the int32 accumulators of nnq.Linear, bias included"""
    return x_q.astype(np.int32) @ w.astype(np.int32).T + bias_q.astype(np.int32)


def linear_q(x_q: np.ndarray, w: np.ndarray, bias_q: np.ndarray, mult) -> np.ndarray:
    """nnq.Linear: x_q (..., K) int8, w (N, K) int8, bias_q (N,) int32 in accumulator units -> (..., N) int8"""
    return requant(linear_acc(x_q, w, bias_q), mult)


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


def mha(x: np.ndarray, t: Dict[str, np.ndarray], H: int = 1, i: int = 0, taps: bool = False, rq=None):
    """x: (B, S, E) float32 block input, or int8 codes x_q; t: the blob-name keyed tensors of params.attention_tensors.
    Returns (out (B, S, E) float32, taps): x_q, Q, K, V, ctx, out_q int8; logits int8 and probs uint8, both
    (B, H, S, S), or (B, S, S) at H = 1 as the engine returns them.  With taps=True a third value: the int32
    accumulators (bias included) of the six requantisation sites, keyed Q, K, V, O (B, S, .) and L (B, H, S, S),
    C (B, H, S, P / H).  rq: a test's stand-in rq(site, acc, mult) -> int8 codes for requant at every site (the block
    itself is rq=None)."""
    g = lambda k: t[f"attn{i}.{k}"]
    sc = np.asarray(g("scal"), np.float32)
    P = g("wq").shape[0]
    if H < 1 or P % H:
        raise ValueError(f"H = {H} does not divide P = {P}")
    rq = rq or (lambda site, acc, m: requant(acc, m))
    x = np.asarray(x)
    x_q = x if x.dtype == np.int8 else quantize(x, sc[INV_SX])
    acc = {k: linear_acc(x_q, g("w" + k.lower()), g("b" + k.lower())) for k in ("Q", "K", "V")}
    Q, K, V = rq("Q", acc["Q"], sc[MQ]), rq("K", acc["K"], sc[MK]), rq("V", acc["V"], sc[MV])
    acc["L"] = split_heads(Q, H).astype(np.int32) @ split_heads(K, H).astype(np.int32).transpose(0, 1, 3, 2)
    logits = rq("L", acc["L"], sc[ML])
    probs = softmax_int(logits)
    B, S, _ = V.shape
    acc["C"] = probs.astype(np.int32) @ split_heads(V, H).astype(np.int32)
    ctx = rq("C", acc["C"], sc[MC]).transpose(0, 2, 1, 3).reshape(B, S, P)
    acc["O"] = linear_acc(ctx, g("wo"), g("bo"))
    out_q = rq("O", acc["O"], sc[MO])
    out = out_q.astype(np.float32) * sc[SO]
    if H == 1:
        logits, probs = logits[:, 0], probs[:, 0]
    tp = dict(x_q=x_q, Q=Q, K=K, V=V, logits=logits, probs=probs, ctx=ctx, out_q=out_q)
    return (out, tp, acc) if taps else (out, tp)


F_INV_SX, M1, M2, S2 = range(4)   # indices of ffn{i}.scal


def ffn(x: np.ndarray, t: Dict[str, np.ndarray], i: int = 0, taps: bool = False, rq=None):
    """ITAFeedForward_QAT: quantise, fc1 + ReLU, fc2, dequantise.  x: (B, S, E) float32 -> (out (B, S, E) float32, taps:
    x_q, h (after the ReLU), out_q int8).  With taps=True a third value: the int32 accumulators fc1 (B, S, F) and fc2
    (B, S, E).  rq: as in mha, with the site names fc1 and fc2."""
    g = lambda k: t[f"ffn{i}.{k}"]
    sc = np.asarray(g("scal"), np.float32)
    rq = rq or (lambda site, acc, m: requant(acc, m))
    x_q = quantize(x, sc[F_INV_SX])
    acc = {"fc1": linear_acc(x_q, g("w1"), g("b1"))}
    h = np.maximum(rq("fc1", acc["fc1"], sc[M1]), 0).astype(np.int8)
    acc["fc2"] = linear_acc(h, g("w2"), g("b2"))
    out_q = rq("fc2", acc["fc2"], sc[M2])
    out = out_q.astype(np.float32) * sc[S2]
    tp = dict(x_q=x_q, h=h, out_q=out_q)
    return (out, tp, acc) if taps else (out, tp)
