"""The float ViT+LSTM graph (models/ITA_single_layer_upsample_shuffle/model.py: float attention with nn.Softmax, float
FFN, nothing quantised) on the CPU: the ITAW0003 blob format (packing, validation by the built plugin, refusal by
consumers that only know ITAW0001), the float-checkpoint export, and the unchanged ITAW0001 / ITAW0002 formats."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, golden_files
from drone_oa_iree_vit_accelerator_amd import params, synth
from float_graph_common import float_state_dict, plugin, repack, unpack, validate  # noqa: F401

ATTN_F32_NAMES = ("attn0.wqf", "attn0.wkf", "attn0.wvf", "attn0.bqf", "attn0.bkf", "attn0.bvf", "attn0.wof", "attn0.bof")
INT8_ATTN_NAMES = ("attn0.wq", "attn0.wk", "attn0.wv", "attn0.wo", "attn0.bq", "attn0.bk", "attn0.bv", "attn0.bo", "attn0.scal")

# sha256 of the blobs these fixtures give under the packer as it was before ITAW0003 existed
UNCHANGED = {
    ("vitlstm_E64_seed0_B2.npz", 1): "b3c0bf8575d935480d2b0e729f8532d340f1f6eb2086ac7340c76cfb8938a23f",
    ("vitlstm_E64_seed1_B2.npz", 1): "a2b685e46ec8762b4f3dd7cd1f776dafb9ec100d575e1d1b3cf31a2a6e817ef9",
    ("onlyattn1l_E64_s0_B2.npz", 1): "9e0d48f1fa2c5d034db9a879eb945e9cc5985ed648bc738c199564151057bbad",
    ("onlyattn2l_E64_s1_B2.npz", 2): "1d79d2ae0087eca9ff15a77b0ba19c494481780fb7b09e7ed403e7c91d75bc95",
}

def test_blob_from_float_params():
    for L in (1, 2):
        fp = synth.float_params(0, E=64, num_layers=L)
        blob = params.blob_from_float_params(fp, L)
        assert blob[:8] == b"ITAW0003"
        assert int(np.frombuffer(blob[32:36], np.int32)[0]) == L
        t = unpack(blob)
        assert not any(n in t for n in INT8_ATTN_NAMES + ("ffn0.w1", "ffn0.scal"))
        for i in range(L):
            a, f = f"attention_blocks.{i}.", f"ffn_blocks.{i}."
            for nm, key in (("q_proj", "q"), ("k_proj", "k"), ("v_proj", "v"), ("out_proj", "o")):
                np.testing.assert_array_equal(t[f"attn{i}.w{key}f"], fp[a + nm + ".weight"])
                np.testing.assert_array_equal(t[f"attn{i}.b{key}f"], fp[a + nm + ".bias"])
            np.testing.assert_array_equal(t[f"ffn{i}.w1f"], fp[f + "fc1.weight"])
            np.testing.assert_array_equal(t[f"ffn{i}.b2f"], fp[f + "fc2.bias"])
        np.testing.assert_array_equal(t["dec.w"], fp["decoder.weight"])
    with pytest.raises(KeyError):
        params.blob_from_float_params({k: v for k, v in synth.float_params(0).items() if "q_proj" not in k})


def test_validate_blob(plugin):
    blob = params.blob_from_float_params(synth.float_params(0))
    assert validate(plugin, blob) == (0, "")
    blob2 = params.blob_from_float_params(synth.float_params(1, num_layers=2), 2)
    assert validate(plugin, blob2) == (0, "")
    t = unpack(blob)
    assert repack(blob, t) == blob   # the repacker is faithful
    for nm in ATTN_F32_NAMES:
        bad_t = dict(t)
        del bad_t[nm]
        rc, bad = validate(plugin, repack(blob, bad_t))
        assert rc != 0 and bad == nm
        bad_t[nm] = t[nm].reshape(-1)[:-4].copy()
        rc, bad = validate(plugin, repack(blob, bad_t))
        assert rc != 0 and bad == nm
        bad_t[nm] = t[nm].astype(np.float16)
        rc, bad = validate(plugin, repack(blob, bad_t))
        assert rc != 0 and bad == nm
    t2 = unpack(blob2)
    del t2["attn1.wkf"]
    rc, bad = validate(plugin, repack(blob2, t2))
    assert rc != 0 and bad == "attn1.wkf"
    # an ITAW0003 blob carrying the int8 attention of an ITAW0002 blob instead of the float one
    d = params.load_fixture(golden_files("onlyattn1l_E64_s0_B2.npz")[0])
    b2 = params.blob_from_record(d, synth.float_params(0, E=64), E=64)
    assert validate(plugin, b2) == (0, "")
    rc, bad = validate(plugin, repack(b2, unpack(b2), magic=b"ITAW0003"))
    assert rc != 0 and bad == "attn0.wqf"
    # and the other way round: float attention under the ITAW0002 magic lacks the int8 attention
    rc, bad = validate(plugin, repack(blob, t, magic=b"ITAW0002"))
    assert rc != 0 and bad == "attn0.wq"


@pytest.mark.parametrize("name,L", sorted(UNCHANGED), ids=lambda v: str(v))
def test_int8_formats_unchanged(plugin, name, L):
    d = params.load_fixture(golden_files(name)[0])
    blob = params.blob_from_record(d, synth.float_params(int(d["meta.seed"]), E=64, num_layers=L), E=64, num_layers=L)
    assert hashlib.sha256(blob).hexdigest() == UNCHANGED[(name, L)]
    assert validate(plugin, blob) == (0, "")


def test_oracle_refuses_float_blob(oracle):
    fx = params.load_fixture(golden_files("floattwin_E64_s0_B2.npz")[0])
    blob = params.blob_from_float_params(synth.float_params(0))
    with pytest.raises(RuntimeError):
        oracle.forward(blob, fx["in0.img_u8"], fx["in0.desvel"], fx["in0.quat"])


@pytest.mark.parametrize("L", [1, 2])
def test_export_float_checkpoint(tmp_path, L):
    sd = float_state_dict(L, 3)
    ck = tmp_path / "model_000205.pth"
    torch.save(sd, str(ck))
    out = tmp_path / "w.itaw"
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "export_blob.py"), "--checkpoint", str(ck),
                        "--out", str(out), "--num-layers", str(L)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    blob = out.read_bytes()
    assert blob[:8] == b"ITAW0003"
    assert blob == params.blob_from_state_dict(sd, L)
    t = unpack(blob)
    want_dec = params.fold_spectral_norm(sd, "decoder")
    np.testing.assert_array_equal(t["dec.w"], want_dec)
    assert not np.array_equal(want_dec, sd["decoder.weight_orig"].numpy())   # the fold is not the identity
    np.testing.assert_array_equal(t["fc.w"], params.fold_spectral_norm(sd, "nn_fc2"))
    for i in range(L):
        np.testing.assert_array_equal(t[f"attn{i}.wqf"], sd[f"attention_blocks.{i}.q_proj.weight"].numpy())
        np.testing.assert_array_equal(t[f"attn{i}.bof"], sd[f"attention_blocks.{i}.out_proj.bias"].numpy())
        np.testing.assert_array_equal(t[f"ffn{i}.w2f"], sd[f"ffn_blocks.{i}.fc2.weight"].numpy())
    # the same blob as the parameters themselves give, with the decoder / fc weights replaced by their folds
    fp = synth.float_params(3, E=64, num_layers=L)
    fp["decoder.weight"], fp["nn_fc2.weight"] = want_dec, params.fold_spectral_norm(sd, "nn_fc2")
    assert blob == params.blob_from_float_params(fp, L)
