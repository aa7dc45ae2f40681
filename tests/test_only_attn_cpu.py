"""The attention-only QAT graph (models/ITA_single_layer_upsample_shuffle/QAT_only_attn/model.py: int8 attention,
float32 FFN + residual + LayerNorm2) on the CPU: its oracle composition against the reference's fixtures, the
ITAW0002 blob format (export, validation, refusal by consumers that only know the int8 FFN)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, golden_files
from drone_oa_iree_vit_accelerator_amd import params, synth
from float_graph_common import converted_state_dict, plugin, unpack, validate  # noqa: F401
from only_attn_common import composed, fp as only_attn_fp, tensors

FIX = golden_files("onlyattn*l_E64_*.npz")


def test_fixtures_present():
    assert len(FIX) == 2 and len(golden_files("onlyattn_qatckpt_E64_s0.npz")) == 1
    for p in FIX + golden_files("onlyattn_qatckpt_*.npz"):
        assert os.path.getsize(p) < 1.2e6


@pytest.mark.parametrize("path", FIX, ids=lambda p: os.path.basename(p)[:-4])
def test_composition_matches_reference(oracle, path):
    d = params.load_fixture(path)
    fp = only_attn_fp(d)
    assert str(d["meta.params_sha256"]) == synth.digest(fp)
    vel0, h0, c0, tp = composed(oracle, d, fp, d["in0.img_u8"], d["in0.desvel"], d["in0.quat"])
    assert np.abs(tp["tokens"] - d["s0.tok.out"]).max() <= 2e-5
    # the int8 codes of every attention block are the reference's (same input codes, same probabilities)
    t = tensors(d, fp)
    x = tp["tokens"]
    for i in range(int(d["meta.num_layers"])):
        _, q = oracle.mha(x, t, i, taps=True)
        np.testing.assert_array_equal(q["x_q"], d[f"s0.attn{i}.x_q"])
        np.testing.assert_array_equal(q["probs"], d[f"s0.attn{i}.probs"].reshape(q["probs"].shape))
        np.testing.assert_array_equal(q["out_q"], d[f"s0.attn{i}.out_q"])
        x = tp[f"x2_{i}"]
    for k in ("x1", "x2", "dec"):
        assert np.abs(tp[k] - d["s0." + k]).max() <= 5e-4, k
    assert np.abs(vel0 - d["s0.vel"]).max() <= 5e-4
    assert np.abs(c0 - d["s0.c"]).max() <= 1e-3
    vel1, h1, c1, _ = composed(oracle, d, fp, d["in1.img_u8"], d["in1.desvel"], d["in1.quat"], h0, c0)
    assert np.abs(vel1 - d["s1.vel"]).max() <= 5e-4
    assert np.abs(h1 - d["s1.h"]).max() <= 1e-3 and np.abs(c1 - d["s1.c"]).max() <= 1e-3


def _only_attn_blob(path=None):
    d = params.load_fixture(path or golden_files("onlyattn1l_E64_s0_B2.npz")[0])
    return d, params.blob_from_record(d, only_attn_fp(d), E=64, num_layers=int(d["meta.num_layers"]))


def test_blob_magic_and_tensors():
    d, blob = _only_attn_blob()
    assert blob[:8] == b"ITAW0002"
    names = _names(blob)
    assert {"ffn0.w1f", "ffn0.b1f", "ffn0.w2f", "ffn0.b2f"} <= set(names)
    assert not any(n in names for n in ("ffn0.w1", "ffn0.w2", "ffn0.b1", "ffn0.b2", "ffn0.scal"))
    # int8 blobs of the existing fixtures: ITAW0001, no float FFN tensor, reserved area zero
    for p in golden_files("vitlstm_*.npz"):
        fx = params.load_fixture(p)
        b = params.blob_from_record(fx, synth.float_params(int(fx["meta.seed"]), E=64), E=64)
        assert b[:8] == b"ITAW0001"
        assert np.frombuffer(b[40:64], np.int32).tolist() == [0] * 6
        assert not any(n.endswith("f") and n.startswith("ffn") for n in _names(b))
    # a record without an int8 FFN needs float FFN parameters
    with pytest.raises(KeyError):
        params.blob_from_record(d, None, E=64)


def _names(blob):
    n = np.frombuffer(blob[8:12], np.int32)[0]
    return [blob[64 + 72 * i: 64 + 72 * i + 32].split(b"\0")[0].decode() for i in range(n)]


def test_export_converted_checkpoint(tmp_path):
    sd = converted_state_dict(golden_files("onlyattn_qatckpt_E64_s0.npz")[0])
    assert "ffn_blocks.0.fc1.weight" in sd and "ffn_blocks.0.fc1._packed_params._packed_params" not in sd
    _, want = _only_attn_blob()      # same seed, same calibration frames
    assert params.blob_from_state_dict(sd) == want
    torch.save(sd, str(tmp_path / "model_quantized_final.pth"))
    out = tmp_path / "w.itaw"
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "export_blob.py"), "--checkpoint",
                        str(tmp_path / "model_quantized_final.pth"), "--out", str(out), "--unsafe-load"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert out.read_bytes() == want


def _retensor(blob, name, dtype=None, shrink=False, drop=False):
    """the same tensors repacked with one of them changed (ITAW0002 kept)"""
    t = unpack(blob)
    if drop:
        del t[name]
    elif shrink:
        t[name] = t[name].reshape(-1)[:-4].copy()
    else:
        t[name] = t[name].astype(dtype)
    return params.pack_blob(t, E=64, num_layers=int(np.frombuffer(blob[32:36], np.int32)[0]), has_tail=True,
                            ffn_f32=blob[:8] == b"ITAW0002")


def test_validate_blob(plugin):
    _, blob = _only_attn_blob()
    assert validate(plugin, blob) == (0, "")
    _, blob2 = _only_attn_blob(golden_files("onlyattn2l_E64_s1_B2.npz")[0])
    assert validate(plugin, blob2) == (0, "")
    assert unpack(blob) and _retensor(blob, "ffn0.w1f", np.float32) == blob   # the repacker is faithful
    for nm in ("ffn0.w1f", "ffn0.b1f", "ffn0.w2f", "ffn0.b2f"):
        rc, bad = validate(plugin, _retensor(blob, nm, shrink=True))
        assert rc != 0 and bad == nm
        rc, bad = validate(plugin, _retensor(blob, nm, dtype=np.float16))
        assert rc != 0 and bad == nm
        rc, bad = validate(plugin, _retensor(blob, nm, drop=True))
        assert rc != 0 and bad == nm
    rc, bad = validate(plugin, _retensor(blob2, "ffn1.w2f", drop=True))
    assert rc != 0 and bad == "ffn1.w2f"
    # an int8 blob still needs its int8 FFN
    fx = params.load_fixture(golden_files("vitlstm_E64_seed0_B2.npz")[0])
    b8 = params.blob_from_record(fx, synth.float_params(0, E=64), E=64)
    assert validate(plugin, b8) == (0, "")
    rc, bad = validate(plugin, _retensor(b8, "ffn0.w2", drop=True))
    assert rc != 0 and bad == "ffn0.w2"


def test_oracle_forward_refuses_float_ffn_blob(oracle):
    d, blob = _only_attn_blob()
    with pytest.raises(RuntimeError):
        oracle.forward(blob, d["in0.img_u8"], d["in0.desvel"], d["in0.quat"])
    # the process is alive and the int8 path still runs
    fx = params.load_fixture(golden_files("vitlstm_E64_seed0_B2.npz")[0])
    b8 = params.blob_from_record(fx, synth.float_params(0, E=64), E=64)
    vel, _, _ = oracle.forward(b8, fx["in0.img_u8"], fx["in0.desvel"], fx["in0.quat"])
    assert np.abs(vel - fx["s0.vel"]).max() <= 5e-4
