"""Histograms of the whole S x S matrix of the float attention block (one head, no 1 / sqrt(d)) in numpy: what
ita_mha_long_f32_hist (Engine.attention_histograms_long_f32) is tested against.  Per frame, with the logits s, the row
maximum m, the row sum l and p = ita_expf(s - m) * (1 / l), every operation rounded to f32 on its own:

    range      (B, 2) f32      minimum and maximum of s
    logits     (B, 256) int64  r = rint(s * scale); bin clamp(r, -128, 127) + 128
    logits_out (B, 2) int64    #{r < -128}, #{r > 127}
    shifts     (B, 256) int64  bin min(rint((m - s) * scale), 255)
    probs      (B, 256) int64  bin bits(p) >> 23: the biased binary exponent of p (127: p = 1; 0: zero and subnormals)

hist_f32 is the definition applied to f32 arrays of the whole matrix (the taps of all rows of Engine.mha_long_f32_taps);
hist64 bins the float64 logits, gaps and probabilities from the parameters the same way and returns those values too, for
a comparison that allows an element near a bin edge to fall on either side.
"""
from __future__ import annotations

from typing import Dict

import numpy as np

from . import attention_stats_f32_ref as asr

NAMES = ("logits", "logits_out", "range", "shifts", "probs")
U8_FLOOR_BIN = 119       # bits(2^-8) >> 23: below it a probability is less than one step of a u8 softmax


def _count(bins: np.ndarray) -> np.ndarray:
    """(B, ...) integer bins in 0 .. 255 -> (B, 256) int64 counts"""
    return np.stack([np.bincount(b.ravel(), minlength=256) for b in bins.astype(np.int64)]).astype(np.int64)


def expf_unique(a: np.ndarray) -> np.ndarray:
    """asr.expf (ita_expf through the oracle's scalar), called once per distinct argument"""
    u, inv = np.unique(np.asarray(a, np.float32), return_inverse=True)
    return asr.expf(u)[inv].reshape(np.shape(a))


def bins_f32(logits: np.ndarray, row_max: np.ndarray, row_sum: np.ndarray, scale: float) -> Dict[str, np.ndarray]:
    """the per-element quantities of the definition: r (f32), and the integer bins of logits, shifts and probs"""
    s, m, l = (np.asarray(v, np.float32) for v in (logits, row_max, row_sum))
    sc = np.float32(scale)
    r = np.rint(s * sc)
    d = m[..., None] - s
    p = expf_unique(s - m[..., None]) * (np.float32(1.0) / l)[..., None]
    assert r.dtype == d.dtype == p.dtype == np.float32
    return dict(r=r, logits=np.clip(r, -128, 127).astype(np.int64) + 128,
                shifts=np.minimum(np.rint(d * sc), np.float32(255)).astype(np.int64),
                probs=(np.ascontiguousarray(p).view(np.uint32) >> 23).astype(np.int64))


def hist_f32(logits: np.ndarray, row_max: np.ndarray, row_sum: np.ndarray, scale: float) -> Dict[str, np.ndarray]:
    """logits (B, S, S), row_max, row_sum (B, S): f32 arrays of the whole matrix -> the five results of NAMES"""
    s = np.asarray(logits, np.float32)
    b = bins_f32(s, row_max, row_sum, scale)
    flat = s.reshape(s.shape[0], -1)
    return dict(logits=_count(b["logits"]), shifts=_count(b["shifts"]), probs=_count(b["probs"]),
                logits_out=np.stack([(b["r"] < -128).sum((1, 2)), (b["r"] > 127).sum((1, 2))], -1).astype(np.int64),
                range=np.stack([flat.min(-1), flat.max(-1)], -1))


def hist64(x: np.ndarray, fp: Dict[str, np.ndarray], scale: float, layer: int = 0) -> Dict[str, np.ndarray]:
    """float64 from the parameters (attention_blocks.<layer>.{q,k}_proj.{weight,bias}): the five results of NAMES binned
    the same way, and the values that were binned: s, d = m - s, p (B, S, S) float64"""
    g = lambda k: np.asarray(fp[f"attention_blocks.{layer}.{k}"], np.float64)
    x = np.asarray(x, np.float64)
    s = (x @ g("q_proj.weight").T + g("q_proj.bias")) @ (x @ g("k_proj.weight").T + g("k_proj.bias")).transpose(0, 2, 1)
    d = s.max(-1, keepdims=True) - s
    e = np.exp(-np.minimum(d, 87.0))            # ita_expf clamps its argument to [-87, 88]: part of the definition of p
    p = e / e.sum(-1, keepdims=True)
    r = np.rint(s * scale)
    mant, ex = np.frexp(p)                      # p = mant 2^ex, mant in [0.5, 1): biased exponent ex + 126
    flat = s.reshape(s.shape[0], -1)
    return dict(logits=_count(np.clip(r, -128, 127) + 128), shifts=_count(np.minimum(np.rint(d * scale), 255)),
                probs=_count(np.where(p < 2.0 ** -126, 0, ex + 126)),
                logits_out=np.stack([(r < -128).sum((1, 2)), (r > 127).sum((1, 2))], -1).astype(np.int64),
                range=np.stack([flat.min(-1), flat.max(-1)], -1), s=s, d=d, p=p)
