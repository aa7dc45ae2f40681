"""Shared by the long float attention tests (test_long_f32_abi.py, test_gpu_long_f32.py): the ITAW0003 blobs, the inputs,
the float64 restatement (attn64 of float_graph_common.py over any S and E, and the whole float layer) and torch's own
f32 result on the CPU, whose error against float64 sets the tests' bound.  Everything cached here is read-only."""
import functools

import numpy as np

from drone_oa_iree_vit_accelerator_amd import float_twin, params, synth

SHAPES = [(128, 3), (256, 2), (384, 2), (1024, 1)]
LAYERS = {64: 1, 128: 2}          # E -> layers of its blob
KINDS = ("plain", "ramp", "ramp_rev", "spike_last", "spike_first")


@functools.lru_cache(maxsize=None)
def case(E):
    """(float parameters, ITAW0003 blob, FloatTwin on the CPU) at E = 64 (one layer) or E = 128 (two layers)"""
    L = LAYERS[E]
    fp = synth.float_params(E, E=E, num_layers=L, tail=(E == 64))
    return fp, params.blob_from_float_params(fp, L), float_twin.FloatTwin(fp, num_layers=L)


def ln_like(B, S, E, seed):
    """LayerNorm-like activations (ln_like of float_graph_common.py): per token zero mean, unit variance, mild affine"""
    rs = np.random.RandomState(seed)
    x = rs.standard_normal((B, S, E))
    x = (x - x.mean(-1, keepdims=True)) / x.std(-1, keepdims=True)
    return (x * (1.0 + 0.1 * rs.standard_normal(E)) + 0.1 * rs.standard_normal(E)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def inputs(kind, E, S, B):
    """plain: ln_like.  ramp: token t times linspace(0.5, 1.5, S)[t], so a row's maximum keeps moving to later key tiles
    and every tile rescales; ramp_rev: reversed, the maximum sits in the first tile and nothing rescales.  spike_last /
    spike_first: one token of 4 x the norm at position S - 1 / 0 -- many rows are one-hot on that key (a fifth of the rows, in float64)."""
    x = ln_like(B, S, E, 7 * S + B + E)
    if kind in ("ramp", "ramp_rev"):
        r = np.linspace(0.5, 1.5, S, dtype=np.float32)
        x = x * (r if kind == "ramp" else r[::-1])[None, :, None]
    elif kind in ("spike_last", "spike_first"):
        x = x.copy()
        x[:, S - 1 if kind == "spike_last" else 0] *= np.float32(4.0)
    elif kind != "plain":
        raise ValueError(kind)
    x = np.ascontiguousarray(x, np.float32)
    x.setflags(write=False)
    return x


def _g(fp, prefix):
    return lambda k: fp[prefix + k].astype(np.float64)


def probs64(x, fp, i):
    """softmax(Q K^T) of ITASelfAttention.forward in float64, and V: one head, no 1 / sqrt(d)"""
    g = _g(fp, f"attention_blocks.{i}.")
    x = x.astype(np.float64)
    q, k, v = (x @ g(f"{n}.weight").T + g(f"{n}.bias") for n in ("q_proj", "k_proj", "v_proj"))
    s = q @ k.transpose(0, 2, 1)
    p = np.exp(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    return p, v


def out_proj64(c, fp, i):
    g = _g(fp, f"attention_blocks.{i}.")
    return c @ g("out_proj.weight").T + g("out_proj.bias")


def attn64(x, fp, i):
    """ITASelfAttention.forward (models/ITA/layers.py:67-88) in float64 over (B, S, E)"""
    p, v = probs64(x, fp, i)
    return out_proj64(p @ v, fp, i)


def _ln64(x, w, b):
    m = x.mean(-1, keepdims=True)
    return (x - m) / np.sqrt(((x - m) ** 2).mean(-1, keepdims=True) + 1e-5) * w.astype(np.float64) + b.astype(np.float64)


def layer64(x, fp, i):
    """LN2(x1 + ffn(x1)), x1 = LN1(x + attn(x)) in float64"""
    f = _g(fp, f"ffn_blocks.{i}.")
    x1 = _ln64(x.astype(np.float64) + attn64(x, fp, i), fp[f"norms1.{i}.weight"], fp[f"norms1.{i}.bias"])
    h = np.maximum(x1 @ f("fc1.weight").T + f("fc1.bias"), 0.0)
    return _ln64(x1 + h @ f("fc2.weight").T + f("fc2.bias"), fp[f"norms2.{i}.weight"], fp[f"norms2.{i}.bias"])


def layer_torch(twin, x, i):
    """the same composition in torch f32 on the CPU (FloatTwin's own layer)"""
    import torch
    F, p, E = torch.nn.functional, twin.p, x.shape[-1]
    with torch.no_grad():
        x = torch.from_numpy(np.array(x, np.float32))
        x1 = F.layer_norm(x + twin._attention(x, i), (E,), p[f"norms1.{i}.weight"], p[f"norms1.{i}.bias"], 1e-5)
        return F.layer_norm(x1 + twin._ffn(x1, i), (E,), p[f"norms2.{i}.weight"], p[f"norms2.{i}.bias"], 1e-5).numpy()


@functools.lru_cache(maxsize=None)
def attn_ref(kind, E, S, B, layer):
    """(float64 attention, e_torch = max |torch CPU f32 attention - float64|) on inputs(kind, E, S, B)"""
    import torch
    fp, _, twin = case(E)
    x = inputs(kind, E, S, B)
    want = attn64(x, fp, layer)
    with torch.no_grad():
        e = float(np.abs(twin._attention(torch.from_numpy(x.copy()), layer).numpy() - want).max())
    want.setflags(write=False)
    return want, e


@functools.lru_cache(maxsize=None)
def layer_ref(kind, E, S, B, layer):
    """(float64 layer, e_torch of the same composition in torch f32) on inputs(kind, E, S, B)"""
    fp, _, twin = case(E)
    x = inputs(kind, E, S, B)
    want = layer64(x, fp, layer)
    e = float(np.abs(layer_torch(twin, x, layer) - want).max())
    want.setflags(write=False)
    return want, e


def bound(e_torch):
    """the project's rule (test_mha_f32_against_float64): three times torch's f32 error on the same rows, never below 1e-5"""
    return max(1e-5, 3.0 * e_torch)
