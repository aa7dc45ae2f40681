"""Multi-head int8 attention on the CPU: the numpy definition (mha_heads_ref) against the pinned C oracle at H = 1 and
against the reference's own multi-head tensors (tests/golden/heads_*.npz, tools/gen_heads_golden.py) at H = 2, 3, 4, 6;
the composed graph against the reference's outputs; the blob's H field."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import heads_common as hc
from conftest import REPO, golden_files
from drone_oa_iree_vit_accelerator_amd import host, mha_heads_ref, params, synth

FIX_H1 = golden_files("blocks_E64_*.npz") + golden_files("blocks_E128_*.npz") + golden_files("vitlstm_E64_seed0_*.npz")


def test_fixtures_present():
    assert sorted(int(hc.case(p)[1]) for p in hc.FIX_HEADS) == [2, 3, 4, 6]
    assert all(hc.heads_of(p) == hc.case(p)[1] for p in hc.FIX_HEADS + hc.FIX_HEADS_2L)   # file name and meta.H agree
    assert len(hc.FIX_HEADS_2L) == 1 and hc.case(hc.FIX_HEADS_2L[0])[1:4] == (4, 128, 2)
    assert len(FIX_H1) == 4


@pytest.mark.parametrize("path", FIX_H1, ids=hc.fixture_id)
def test_one_head_equals_the_oracle(oracle, path):
    """ties the numpy definition to the pinned C oracle: every tap and the f32 output, bit for bit"""
    d = params.load_fixture(path)
    t = params.attention_tensors(d, "attn0.", 0)
    x = d["s0.attn0.x_q.in"]
    want, wt = oracle.mha(x, t, taps=True)
    got, gt = mha_heads_ref.mha(x, t, H=1)
    assert set(gt) == set(wt)
    for k in wt:
        assert gt[k].dtype == wt[k].dtype and gt[k].shape == wt[k].shape, k
        np.testing.assert_array_equal(gt[k], wt[k], err_msg=k)
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got, want)
    # int8 codes in: the same block behind the quantiser
    got8, _ = mha_heads_ref.mha(wt["x_q"], t, H=1)
    np.testing.assert_array_equal(got8, want)


@pytest.mark.parametrize("path", hc.FIX_HEADS, ids=hc.fixture_id)
def test_stages_equal_the_reference(path):
    """every stage from the reference's own input of that stage: bit for bit, except matmul1's documented near-ties
    (the reference's float fallback: <= 3 logits per fixture, each within 2e-4 of a rounding tie)"""
    d, H, E, nl, t, fp, blob = hc.case(path)
    sc = t["attn0.scal"]
    out, tp = mha_heads_ref.mha(d["s0.attn0.x_q.in"], t, H)
    for k, ref in (("x_q", "x_q"), ("Q", "Q"), ("K", "K"), ("V", "V")):
        np.testing.assert_array_equal(tp[k], d["s0.attn0." + ref], err_msg=k)
    ref_l = d["s0.attn0.probs.in"]
    assert ref_l.shape == (tp["Q"].shape[0], H, 128, 128)
    ours, acc = mha_heads_ref.logits_from(d["s0.attn0.Q"], d["s0.attn0.K"], H, sc[mha_heads_ref.ML])
    bad = np.argwhere(ours != ref_l)
    print(f"{hc.fixture_id(path)}: {len(bad)} logits differ from the reference")
    assert len(bad) <= 3
    for i in map(tuple, bad):
        exact = float(acc[i]) * float(sc[mha_heads_ref.ML])
        assert abs(abs(exact - np.floor(exact)) - 0.5) < 2e-4 and abs(int(ours[i]) - int(ref_l[i])) == 1
    np.testing.assert_array_equal(mha_heads_ref.softmax_int(ref_l), d["s0.attn0.probs"])
    ctx = mha_heads_ref.ctx_from(d["s0.attn0.probs"], d["s0.attn0.V"], H, sc[mha_heads_ref.MC])
    np.testing.assert_array_equal(ctx, d["s0.attn0.out_q.in"])
    out_q = mha_heads_ref.linear_q(d["s0.attn0.out_q.in"], t["attn0.wo"], t["attn0.bo"], sc[mha_heads_ref.MO])
    np.testing.assert_array_equal(out_q, d["s0.attn0.out_q"])
    np.testing.assert_array_equal(out_q.astype(np.float32) * sc[mha_heads_ref.SO], d["s0.attn0.out_f"])
    if not len(bad):   # no near-tie logit: the whole block from the float input is the reference's
        np.testing.assert_array_equal(tp["logits"], ref_l)
        np.testing.assert_array_equal(tp["probs"], d["s0.attn0.probs"])
        np.testing.assert_array_equal(tp["ctx"], d["s0.attn0.out_q.in"])
        np.testing.assert_array_equal(out, d["s0.attn0.out_f"])


GRAPHS = hc.FIX_GRAPHS


@pytest.mark.parametrize("path", GRAPHS, ids=hc.fixture_id)
def test_graph_from_reference_tokens(oracle, path):
    """the whole graph behind the tokenizer, composed around mha_heads_ref, against the reference's outputs of the same
    forward: the bounds of test_oracle_golden.py::test_forward_from_reference_tokens (velocity 1e-5, h and c 5e-4)"""
    d, H, E, nl, t, fp, blob = hc.case(path)
    vel, h, c, x2 = hc.forward_from_tokens(oracle, d["s0.tok.out"], t, fp, nl, H, d["in0.desvel"], d["in0.quat"])
    x2_ref = d[f"s0.x2_{nl - 1}"] if f"s0.x2_{nl - 1}" in d else d["s0.x2"]
    for name, got, ref in (("x2", x2, x2_ref), ("vel", vel, d["s0.vel"]), ("h", h, d["s0.h"]), ("c", c, d["s0.c"])):
        print(f"{hc.fixture_id(path)}: max |{name} - reference| = {np.abs(got - ref).max():.3e}")
    np.testing.assert_allclose(vel, d["s0.vel"], atol=1e-5, rtol=0)
    np.testing.assert_allclose(h, d["s0.h"], atol=5e-4, rtol=0)
    np.testing.assert_allclose(c, d["s0.c"], atol=5e-4, rtol=0)


def test_blob_header_carries_the_head_count(tmp_path):
    lib = host.lib()
    lib.ita_validate_blob.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p]
    d = params.load_fixture(golden_files("vitlstm_E64_seed0_B2.npz")[0])
    fp = synth.float_params(0, E=64)
    t = {**params.attention_tensors(d, "attn0.", 0), **params.ffn_tensors(d, "ffn0.", 0), **params.float_tensors(fp)}
    bad = ctypes.create_string_buffer(32)
    blob = params.pack_blob(t, E=64, H=3)
    assert lib.ita_validate_blob(blob, len(blob), bad) == 0
    assert int(np.frombuffer(blob[28:32], np.int32)[0]) == 3
    rec3, one = params.blob_from_record(d, fp, E=64, H=3), params.blob_from_record(d, fp, E=64)
    assert lib.ita_validate_blob(rec3, len(rec3), bad) == 0
    assert int(np.frombuffer(rec3[28:32], np.int32)[0]) == 3 and int(np.frombuffer(one[28:32], np.int32)[0]) == 1
    assert rec3[:28] == one[:28] and rec3[32:] == one[32:]   # nothing else depends on the head count
    # a head is a whole number of 16-feature chunks of P = 192; a header H whose multiple of 16 wraps around in 32 bits
    # (2^28: 16 H = 0, 2^27 + 1, INT_MAX) or is negative is refused like any other, without dividing by it
    for H in (5, 0, 24, -1, -3, 1 << 28, (1 << 27) + 1, (1 << 28) + 3, 0x7fffffff, -(1 << 31)):
        b = params.pack_blob(t, E=64, H=H)
        assert lib.ita_validate_blob(b, len(b), bad) != 0, H
    # the command line: a state dict does not hold the head count
    from float_graph_common import converted_state_dict
    torch.save(converted_state_dict(golden_files("qatckpt_E64_s0.npz")[0]), str(tmp_path / "ckpt.pth"))
    out = tmp_path / "w.itaw"
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "export_blob.py"), "--checkpoint", str(tmp_path / "ckpt.pth"),
                        "--out", str(out), "--heads", "3", "--unsafe-load"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert out.read_bytes() == rec3
