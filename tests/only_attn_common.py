"""The attention-only QAT graph's float parameters, blob-name keyed tensors and oracle composition, shared by
test_only_attn_cpu.py and the GPU tests that load an onlyattn* fixture.  CPU only."""
import numpy as np

from conftest import golden_files
from drone_oa_iree_vit_accelerator_amd import params, synth


def fp(d):
    return synth.float_params(int(d["meta.seed"]), E=64, num_layers=int(d["meta.num_layers"]))


def tensors(d, fp):
    """blob-name keyed tensors of the attention-only graph (what blob_from_record packs)"""
    L = int(d["meta.num_layers"])
    t = {}
    for i in range(L):
        t.update(params.attention_tensors(d, f"attn{i}.", i))
    t.update(params.float_tensors(fp, L))
    return t


def composed(oracle, d, fp, image, desvel, quat, h_in=None, c_in=None):
    """oracle.tokenizer -> per layer mha + add_ln (LN1), linear_f32 / ReLU / linear_f32 + add_ln (LN2) -> tail ->
    linear_f32 -> head_from_dec.  Returns (vel, h, c, taps)."""
    L = int(d["meta.num_layers"])
    t = tensors(d, fp)
    x = oracle.tokenizer(image, t["tok.conv_w"], t["tok.conv_b"], t["tok.ln_w"], t["tok.ln_b"])
    tp = {"tokens": x}
    for i in range(L):
        x1 = oracle.add_ln(x, oracle.mha(x, t, i), t[f"norm1_{i}.w"], t[f"norm1_{i}.b"])
        hid = np.maximum(oracle.linear_f32(x1, t[f"ffn{i}.w1f"], t[f"ffn{i}.b1f"]), np.float32(0))
        x = oracle.add_ln(x1, oracle.linear_f32(hid, t[f"ffn{i}.w2f"], t[f"ffn{i}.b2f"]), t[f"norm2_{i}.w"], t[f"norm2_{i}.b"])
        tp[f"x1_{i}"], tp[f"x2_{i}"] = x1, x
    tp["x1"], tp["x2"] = tp[f"x1_{L - 1}"], x
    tp["feat"] = oracle.tail(x, t["tail.conv_w"], t["tail.conv_b"])
    tp["dec"] = oracle.linear_f32(tp["feat"], t["dec.w"], t["dec.b"])
    vel, h, c = oracle.head_from_dec(tp["dec"], desvel, quat, fp, h_in, c_in)
    return vel, h, c, tp


FIX = {1: golden_files("onlyattn1l_E64_s0_B2.npz")[0], 2: golden_files("onlyattn2l_E64_s1_B2.npz")[0]}


def setup_only_attn(L):
    d = params.load_fixture(FIX[L])
    p = fp(d)
    return d, p, params.blob_from_record(d, p, E=64, num_layers=L)
