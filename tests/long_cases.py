"""The long int8 tests' fixtures and input generators, shared by the CPU and the GPU tests.  CPU only.

Three generators, kept apart because every expectation is computed from what they give:
    long_inputs   int8 codes in blocks of 32 similar tokens
    long_f32      f32 tokens that quantise to long_inputs' codes; the sub-code offset u comes from a stream of its own
                  (seed + 1000)
    tokens        f32 tokens of the same kind with u drawn from the one stream that gave the codes"""
import functools
from typing import NamedTuple, Optional

import numpy as np

from conftest import golden_files
from drone_oa_iree_vit_accelerator_amd import params, synth
from only_attn_common import fp as only_attn_fp

INV_SX = 0
# name -> does the layer run the FAST (single-rounding) instantiation
FIXTURES = {"vitlstm_E64_seed0_B2": True, "vitlstm_E64_seed1_B2": False, "blocks_E128_seed0_B1": False,
            "vit2l_us_E128_s1_B2": True, "onlyattn1l_E64_s0_B2": None}
TWO_LAYER = "vit2l_E128_s0_B2"


class LongCase(NamedTuple):
    E: int
    num_layers: int
    t: dict                 # the attention tensors of every layer, and the FFN tensors where the record has an int8 FFN
    fp: Optional[dict]      # the float parameters: of a vit* or an onlyattn* record, else None
    blob: bytes


@functools.lru_cache(maxsize=None)
def long_case(name):
    """one fixture of tests/golden; read-only"""
    d = params.load_fixture(golden_files(name + ".npz")[0])
    E = int(d["meta.E"])
    nl = int(d["meta.num_layers"]) if "meta.num_layers" in d else 1
    if name.startswith("onlyattn"):
        fp = only_attn_fp(d)
    else:
        fp = synth.float_params(int(d["meta.seed"]), E=E, num_layers=nl, tail=(E == 64)) if name.startswith("vit") else None
    t = {}
    for l in range(nl):
        t.update(params.attention_tensors(d, f"attn{l}.", l))
        if "ffn0.fc1.w_q" in d:
            t.update(params.ffn_tensors(d, f"ffn{l}.", l))
    return LongCase(E, nl, t, fp, params.blob_from_record(d, fp, E=E, num_layers=nl))


def tokens(seed, B, S, E, t, l=0):
    """f32 tokens in blocks of 32 similar ones (all-noise rows make the integer softmax degenerate), off the code grid"""
    rs = np.random.RandomState(seed)
    base = rs.standard_normal((B, S // 32, E)).repeat(32, axis=1) * 18.0
    codes = np.clip(np.rint(base + rs.standard_normal((B, S, E)) * 9.0), -128, 127).astype(np.float32)
    u = rs.uniform(-0.4, 0.4, size=codes.shape).astype(np.float32)
    return ((codes + u) * (np.float32(1.0) / np.float32(t[f"attn{l}.scal"][INV_SX]))).astype(np.float32)


def tap_rows(S):
    """the query rows the taps are read at: two in one wave, waves with none, the first and the last, two query tiles"""
    return sorted({0, 1, 15, 16, 17, 127, 128 % S, S - 1})


def long_inputs(seed, B, S, E):
    """structured codes: blocks of 32 similar tokens (all-noise rows make the integer softmax degenerate)"""
    rs = np.random.RandomState(seed)
    base = rs.standard_normal((B, S // 32, E)).repeat(32, axis=1) * 18.0
    x = base + rs.standard_normal((B, S, E)) * 9.0
    return np.clip(np.rint(x), -128, 127).astype(np.int8)


def long_f32(seed, B, S, E, t, l=0):
    """f32 tokens that quantise to those codes: (codes + u) * s_x, u uniform in (-0.4, 0.4), s_x = 1 / scal[INV_SX]"""
    codes = long_inputs(seed, B, S, E).astype(np.float32)
    u = np.random.RandomState(seed + 1000).uniform(-0.4, 0.4, size=codes.shape).astype(np.float32)
    s_x = np.float32(1.0) / np.float32(t[f"attn{l}.scal"][INV_SX])
    return ((codes + u) * s_x).astype(np.float32)
