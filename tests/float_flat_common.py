"""Shared by the flat-softmax tests of the float attention (test_float_flat_cpu.py, test_gpu_float_flat.py).

With the synthetic weights every other test uses, softmax(Q K^T) without 1/sqrt(d) is close to a hard maximum: the median
row has two or three keys above 1e-4, so P V is in effect a gather of one V row.  Here q_proj (weight and bias) of the layer
under test is multiplied by s in SCALES, which flattens the rows: at s = 0 every probability is exactly 1 / S, at 1 / 64
every key of every row counts, at 1 / 8 a few dozen do.  The float64 definitions, the inputs and the bound are those of
long_f32_common.py; nothing is restated.  Everything cached here is read-only."""
import functools

import numpy as np

from drone_oa_iree_vit_accelerator_amd import float_twin, params
import long_f32_common as lc
from long_f32_common import LAYERS

SCALES = (0.0, 1.0 / 64, 1.0 / 8)
KINDS = ("plain", "ramp")
SHORT = (128, 3)                    # (S, B) of mha_f32 / encoder_layer
LONG = ((256, 2), (384, 2))         # (S, B) of mha_long_f32: 4 and 6 units of 64 keys
P_MIN = 1e-4                        # a key "counts" in a row when its probability is above this


def label(s):
    return "0" if s == 0 else f"1/{round(1 / s)}"


@functools.lru_cache(maxsize=None)
def case(E, layer, s):
    """(float parameters, ITAW0003 blob, FloatTwin) of long_f32_common.case(E) with q_proj of `layer` times s; s = 1 is
    the stock case itself"""
    if s == 1:
        return lc.case(E)
    fp = dict(lc.case(E)[0])
    for k in ("weight", "bias"):
        name = f"attention_blocks.{layer}.q_proj.{k}"
        fp[name] = (fp[name] * np.float32(s)).astype(np.float32)
    return fp, params.blob_from_float_params(fp, LAYERS[E]), float_twin.FloatTwin(fp, num_layers=LAYERS[E])


def keys_per_row(x, fp, layer):
    """number of keys with probability above P_MIN in each row of the float64 softmax, (B, S) ints"""
    return (lc.probs64(x, fp, layer)[0] > P_MIN).sum(-1)


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def attn_ref(kind, E, S, B, layer, s):
    """(float64 attention, e_torch = max |torch CPU f32 attention - float64|) on lc.inputs(kind, E, S, B) with case(E, layer, s)"""
    import torch
    fp, _, twin = case(E, layer, s)
    x = lc.inputs(kind, E, S, B)
    want = lc.attn64(x, fp, layer)
    with torch.no_grad():
        e = float(np.abs(twin._attention(torch.from_numpy(x.copy()), layer).numpy() - want).max())
    return _frozen(want), e


@functools.lru_cache(maxsize=None)
def layer_ref(kind, E, S, B, layer, s):
    """(float64 layer, e_torch of the same composition in torch f32) on lc.inputs(kind, E, S, B) with case(E, layer, s)"""
    fp, _, twin = case(E, layer, s)
    x = lc.inputs(kind, E, S, B)
    want = lc.layer64(x, fp, layer)
    e = float(np.abs(lc.layer_torch(twin, x, layer) - want).max())
    return _frozen(want), e


def duplicated(E):
    """lc.inputs('plain', E, *SHORT) with token 3 copied to tokens 77 and 120: the same query in waves 0, 4 and 7"""
    x = lc.inputs("plain", E, *SHORT).copy()
    x[:, 77] = x[:, 3]
    x[:, 120] = x[:, 3]
    return _frozen(x)


def attn64_without_key_tile(x, fp, layer, kt):
    """lc.attn64 with the 16 keys of tile kt left out of the context GEMM (the probabilities still sum over all keys):
    the fault `skip key tile kt` of the kernel's ctx^T = V^T P^T loop, restated in float64"""
    p, v = lc.probs64(x, fp, layer)
    p = p.copy()
    p[:, :, 16 * kt:16 * kt + 16] = 0.0
    return lc.out_proj64(p @ v, fp, layer)
