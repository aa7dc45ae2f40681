"""Attention rollout (Abnar & Zuidema, 2020) over int8 attention layers with H heads, in numpy: the definition
Engine.attention_rollout_long_heads is tested against.  attention_rollout_ref's recurrence with the attention matrix of a
layer taken as the mean of its heads, (1 / H) sum_hd P_l,hd / 256:

    s = max_j v[j]  (1 where that is 0)
    q = rint((v / s) * 2097151)                              int64, 21 bits
    v <- 0.5 * (v + ((float64(sum_hd q @ P_l,hd) * (s / 2097151)) / (256 * H)))

The sum over the heads is an exact integer (below 2^21 * 255 * 65536 * 6 < 2^53, so its float64 is exact too) and every
other step is ONE correctly rounded float64 operation in the order the brackets give, so two implementations agree bit for
bit.  At H = 1 this is attention_rollout_ref.rollout.

The layers are composed as tests/heads_common.encoder_layer composes them: attention by mha_heads_ref with H heads,
residual + LayerNorm and the FFN by the C oracle, which the caller hands in (this package does not import it).
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np

from . import attention_propagate_heads_ref as aphr
from . import mha_heads_ref as ref
from .attention_rollout_ref import QMAX, start


def layer_inputs(oracle, x: np.ndarray, t: Dict[str, np.ndarray], fp, num_layers: int, H: int, first_layer: int = 0):
    """[x_l for l in first_layer .. num_layers - 1]: the token rows entering each layer, x entering first_layer"""
    xs = [np.ascontiguousarray(x, np.float32)]
    for l in range(first_layer, num_layers - 1):
        a, _ = ref.mha(xs[-1], t, H, l)
        x1 = oracle.add_ln(xs[-1], a, fp[f"norms1.{l}.weight"], fp[f"norms1.{l}.bias"])
        xs.append(oracle.add_ln(x1, oracle.ffn(x1, t, l), fp[f"norms2.{l}.weight"], fp[f"norms2.{l}.bias"]))
    return xs


def step(v: np.ndarray, x: np.ndarray, t: Dict[str, np.ndarray], H: int, l: int) -> np.ndarray:
    """one layer of the recurrence: v (B, n, S) float64, x the token rows entering layer l"""
    s = v.max(-1, keepdims=True)
    s = np.where(s == 0, 1.0, s)
    q = np.rint((v / s) * float(QMAX)).astype(np.int64)
    qp = aphr.propagate_heads64(x, t, q, H, l).sum(1)
    return 0.5 * (v + ((qp.astype(np.float64) * (s / float(QMAX))) / (256.0 * H)))


def rollout(oracle, x: np.ndarray, t: Dict[str, np.ndarray], fp, num_layers: int, H: int,
            rows: Optional[Sequence[int]] = None, first_layer: int = 0) -> np.ndarray:
    """x: (B, S, E) float32 token rows entering first_layer -> float64 (B, n, S)"""
    xs = layer_inputs(oracle, x, t, fp, num_layers, H, first_layer)
    v = start(x.shape[0], x.shape[1], rows)
    for l in range(num_layers - 1, first_layer - 1, -1):
        v = step(v, xs[l - first_layer], t, H, l)
    return v
