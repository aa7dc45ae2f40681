"""Shared by test_heads_cpu.py and test_gpu_heads.py: the multi-head fixtures and the graph composed around
mha_heads_ref (the C oracle has one head; every other stage is the oracle's)."""
import functools
import re

import numpy as np

from conftest import golden_files
from drone_oa_iree_vit_accelerator_amd import mha_heads_ref, params, synth

FIX_HEADS = golden_files("heads_E64_H*_s0_B*.npz")        # the whole ITAViTLSTM graph, H = 2, 3, 4, 6
FIX_HEADS_2L = golden_files("heads2l_E128_H4_s0_B*.npz")  # E = 128, two layers, no fusion tail, H = 4


def fixture_id(path):
    return path.rsplit("/", 1)[-1][:-4]


def heads_of(path):
    """the head count in a fixture's file name (..._H3_...): lets a module pick its cases without loading a file"""
    return int(re.search(r"_H(\d+)_", fixture_id(path)).group(1))


FIX_GRAPHS = [p for p in FIX_HEADS if heads_of(p) == 3] + FIX_HEADS_2L   # the whole-graph cases: E = 64 H = 3, E = 128 H = 4


@functools.lru_cache(maxsize=None)
def case(path):
    """(fixture record, H, E, num_layers, block tensors, float parameters, blob) of one fixture; read-only"""
    d = params.load_fixture(path)
    H, E = int(d["meta.H"]), int(d["meta.E"])
    nl = int(d["meta.num_layers"]) if "meta.num_layers" in d else 1
    fp = synth.float_params(int(d["meta.seed"]), E=E, num_layers=nl, tail=(E == 64))
    t = {}
    for l in range(nl):
        t.update(params.attention_tensors(d, f"attn{l}.", l))
        t.update(params.ffn_tensors(d, f"ffn{l}.", l))
    blob = params.blob_from_record(d, fp, E=E, num_layers=nl, H=H)
    return d, H, E, nl, t, fp, blob


def encoder_layer(oracle, x, t, fp, H, l=0):
    """(x1, x2) of one encoder layer: attention with H heads, residual + LayerNorm1, FFN, residual + LayerNorm2"""
    a, _ = mha_heads_ref.mha(x, t, H, l)
    x1 = oracle.add_ln(x, a, fp[f"norms1.{l}.weight"], fp[f"norms1.{l}.bias"])
    x2 = oracle.add_ln(x1, oracle.ffn(x1, t, l), fp[f"norms2.{l}.weight"], fp[f"norms2.{l}.bias"])
    return x1, x2


def encoder(oracle, tokens, t, fp, nl, H):
    """all nl encoder layers -> (the LAST layer's LayerNorm1 output x1, what the engine's x1 tap holds, and x2)"""
    x, x1 = np.ascontiguousarray(tokens, np.float32), None
    for l in range(nl):
        x1, x = encoder_layer(oracle, x, t, fp, H, l)
    return x1, x


def forward_from_tokens(oracle, tokens, t, fp, nl, H, desvel, quat, h_in=None, c_in=None):
    """oracle.forward_from_tokens with mha_heads_ref as the attention block -> (vel, h, c, x2)"""
    _, x = encoder(oracle, tokens, t, fp, nl, H)
    B = x.shape[0]
    if "down_sample.weight" in fp:
        feat = oracle.tail(x, fp["down_sample.weight"], fp["down_sample.bias"])
    else:
        feat = x.reshape(B, -1)
    dec = oracle.linear_f32(feat, fp["decoder.weight"], fp["decoder.bias"])
    vel, h, c = oracle.head_from_dec(dec, desvel, quat, fp, h_in, c_in)
    return vel, h, c, x


def forward(oracle, img, t, fp, nl, H, desvel, quat, h_in=None, c_in=None):
    """the same from u8 or f32 frames, behind the oracle's tokenizer (what oracle.forward composes at H = 1)"""
    tokens = oracle.tokenizer(img, fp["tokenizer.conv.weight"], fp["tokenizer.conv.bias"], fp["tokenizer.norm.weight"],
                              fp["tokenizer.norm.bias"])
    return forward_from_tokens(oracle, tokens, t, fp, nl, H, desvel, quat, h_in, c_in)[:3]
