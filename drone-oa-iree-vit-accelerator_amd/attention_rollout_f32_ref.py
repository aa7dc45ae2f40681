"""Attention rollout (Abnar & Zuidema, "Quantifying Attention Flow in Transformers", 2020) over float-attention layers at
H = 1, in numpy float64: the definition Engine.attention_rollout_long_f32 is tested against.

Identity residual, attention matrix P_l = softmax(Q K^T) of layer l from the token rows x_l entering the layer.  A row
vector v (what an output token depends on) walks from the last layer down to first_layer:

    v <- 0.5 * (v + v @ P_l)

v starts as one-hot(rows), or as the single vector 1 / S (attention_rollout_ref.start, restated here so that this file
imports nothing but numpy and attention_propagate_f32_ref).  Every P_l is row-stochastic, so every v stays non-negative
and keeps the sum 1.  The caller hands in the layer inputs xs (float64 or f32 rows, tests/long_f32_common.layer64 builds
them): this package composes no float layer in numpy.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np

from . import attention_propagate_f32_ref as apr


def start(B: int, S: int, rows: Optional[Sequence[int]]) -> np.ndarray:
    """one-hot(rows) (B, len(rows), S), or the single vector 1 / S"""
    if rows is None:
        return np.full((B, 1, S), 1.0 / S, np.float64)
    v = np.zeros((B, len(rows), S), np.float64)
    for n, r in enumerate(rows):
        v[:, n, r] = 1.0
    return v


def rollout64(xs: Sequence[np.ndarray], fp: Dict[str, np.ndarray], rows: Optional[Sequence[int]] = None,
              first_layer: int = 0, block: int = 1024) -> np.ndarray:
    """xs: [x_l for l in first_layer .. first_layer + len(xs) - 1], each (B, S, E): the token rows entering each layer
    -> float64 (B, n, S)"""
    B, S = xs[0].shape[0], xs[0].shape[1]
    v = start(B, S, rows)
    for l in range(first_layer + len(xs) - 1, first_layer - 1, -1):
        v = 0.5 * (v + apr.propagate64(xs[l - first_layer], fp, v, l, block))
    return v
