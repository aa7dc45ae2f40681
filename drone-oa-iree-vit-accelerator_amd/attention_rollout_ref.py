"""Attention rollout (Abnar & Zuidema, "Quantifying Attention Flow in Transformers", 2020) over the int8 attention layers
at H = 1, in numpy: the definition Engine.attention_rollout_long is tested against.

Identity residual, attention matrix P_l / 256 with P_l the uint8 probabilities (S x S) of layer l that mha_heads_ref
computes from the token rows x_l entering the layer.  A row vector v (what an output token depends on) walks from the
last layer down to first_layer:

    s = max_j v[j]  (1 where that is 0)
    q = rint((v / s) * 2097151)                              int64, 21 bits
    v <- 0.5 * (v + ((float64(q @ P_l) * (s / 2097151)) / 256))

q @ P_l is an exact integer (below 2^21 * 255 * 65536 < 2^53, so its float64 is exact too) and every other step is ONE
correctly rounded float64 operation in the order the brackets give, so two implementations agree bit for bit.  v starts as
one-hot(rows), or as the single vector 1 / S.

The layers are composed as tests/heads_common.encoder_layer composes them with H = 1: attention by mha_heads_ref, residual
+ LayerNorm and the FFN by the C oracle, which the caller hands in (this package does not import it).
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np

from . import attention_propagate_ref as apr
from . import mha_heads_ref as ref

QMAX = 2097151          # 2^21 - 1


def layer_inputs(oracle, x: np.ndarray, t: Dict[str, np.ndarray], fp, num_layers: int, first_layer: int = 0):
    """[x_l for l in first_layer .. num_layers - 1]: the token rows entering each layer, x entering first_layer"""
    xs = [np.ascontiguousarray(x, np.float32)]
    for l in range(first_layer, num_layers - 1):
        a, _ = ref.mha(xs[-1], t, 1, l)
        x1 = oracle.add_ln(xs[-1], a, fp[f"norms1.{l}.weight"], fp[f"norms1.{l}.bias"])
        xs.append(oracle.add_ln(x1, oracle.ffn(x1, t, l), fp[f"norms2.{l}.weight"], fp[f"norms2.{l}.bias"]))
    return xs


def start(B: int, S: int, rows: Optional[Sequence[int]]) -> np.ndarray:
    """one-hot(rows) (B, len(rows), S), or the single vector 1 / S"""
    if rows is None:
        return np.full((B, 1, S), 1.0 / S, np.float64)
    v = np.zeros((B, len(rows), S), np.float64)
    for n, r in enumerate(rows):
        v[:, n, r] = 1.0
    return v


def step(v: np.ndarray, x: np.ndarray, t: Dict[str, np.ndarray], l: int) -> np.ndarray:
    """one layer of the recurrence: v (B, n, S) float64, x the token rows entering layer l"""
    s = v.max(-1, keepdims=True)
    s = np.where(s == 0, 1.0, s)
    q = np.rint((v / s) * float(QMAX)).astype(np.int64)
    qp = apr.propagate64(x, t, q, l)
    return 0.5 * (v + ((qp.astype(np.float64) * (s / float(QMAX))) / 256.0))


def rollout(oracle, x: np.ndarray, t: Dict[str, np.ndarray], fp, num_layers: int, rows: Optional[Sequence[int]] = None,
            first_layer: int = 0) -> np.ndarray:
    """x: (B, S, E) float32 token rows entering first_layer -> float64 (B, n, S)"""
    xs = layer_inputs(oracle, x, t, fp, num_layers, first_layer)
    v = start(x.shape[0], x.shape[1], rows)
    for l in range(num_layers - 1, first_layer - 1, -1):
        v = step(v, xs[l - first_layer], t, l)
    return v
