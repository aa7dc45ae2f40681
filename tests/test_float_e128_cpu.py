"""The float graphs without the fusion tail on the CPU: ITALSTMNetVIT of models/ITA_upsample_shuffle/model.py (E = 128,
two layers, decoder 16384 -> 512) and ITALSTMNetVIT_single_layer of models/ITA_single_layer/model.py (E = 64, one
layer, decoder 8192 -> 512).  FloatTwin against the reference's own modules (tests/golden/floatnt*), their ITAW0003 blobs,
and the export of a checkpoint in each model file's state_dict layout."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, golden_files
from drone_oa_iree_vit_accelerator_amd import float_twin, params, synth
from float_graph_common import Attention, Ffn, Tokenizer, unpack, validate, plugin  # noqa: F401

GRAPHS = {128: ("floatnt2l_E128_s1_B2.npz", 2), 64: ("floatnt1l_E64_s2_B2.npz", 1)}


def _setup(E):
    name, L = GRAPHS[E]
    d = params.load_fixture(golden_files(name)[0])
    fp = synth.float_params(int(d["meta.seed"]), E=E, num_layers=L, tail=False)
    assert str(d["meta.params_sha256"]) == synth.digest(fp)
    assert int(d["meta.E"]) == E and int(d["meta.num_layers"]) == L
    return d, fp, L


@pytest.mark.parametrize("E", [128, 64])
def test_float_twin_against_reference(E):
    d, fp, L = _setup(E)
    twin = float_twin.FloatTwin(fp, num_layers=L)
    v0, (h0, c0), tp = twin.forward(d["in0.img_u8"], d["in0.desvel"], d["in0.quat"], taps=True)
    v1, (h1, c1) = twin.forward(d["in1.img_u8"], d["in1.desvel"], d["in1.quat"], hidden=(h0, c0))
    got = {"tok.out": tp["tokens"], "dec": tp["dec"], "vel": v0, "h": h0, "c": c0}
    for i in range(L):
        got[f"x1_{i}"], got[f"x2_{i}"] = tp[f"x1_{i}"], tp[f"x2_{i}"]
    for k, v in got.items():
        err = np.abs(v.numpy() - d["s0." + k]).max()
        assert err <= 1e-5, (k, err)
    for k, v in (("vel", v1), ("h", h1), ("c", c1)):
        err = np.abs(v.numpy() - d["s1." + k]).max()
        assert err <= 1e-5, (k, err)


@pytest.mark.parametrize("E", [128, 64])
def test_blob_without_tail(plugin, E):  # noqa: F811
    _, fp, L = _setup(E)
    blob = params.blob_from_float_params(fp, L)
    assert blob[:8] == b"ITAW0003"
    hdr = np.frombuffer(blob[12:44], np.int32)
    assert int(hdr[0]) == E and int(hdr[5]) == L and int(hdr[6]) == 0   # E, num_layers, has_tail
    t = unpack(blob)
    assert not [k for k in t if k.startswith("tail.")]
    assert t["dec.w"].shape == (512, E * 128)
    np.testing.assert_array_equal(t["dec.w"], fp["decoder.weight"])
    assert validate(plugin, blob) == (0, "")


class _UpsampleShuffleNet(torch.nn.Module):
    """models/ITA_upsample_shuffle/model.py's parameter tree: two layers under norm1_layers / norm2_layers, the unused
    down_sample Conv2d(160, 48, 3), decoder and nn_fc2 under spectral_norm"""

    def __init__(self, E=128, P=192, F=256):
        super().__init__()
        self.tokenizer = Tokenizer(E)
        self.attention_blocks = torch.nn.ModuleList(Attention(E, P) for _ in range(2))
        self.ffn_blocks = torch.nn.ModuleList(Ffn(E, F) for _ in range(2))
        self.norm1_layers = torch.nn.ModuleList(torch.nn.LayerNorm(E) for _ in range(2))
        self.norm2_layers = torch.nn.ModuleList(torch.nn.LayerNorm(E) for _ in range(2))
        self.decoder = torch.nn.utils.spectral_norm(torch.nn.Linear(E * 128, 512))
        self.lstm = torch.nn.LSTM(input_size=517, hidden_size=128, num_layers=3)
        self.nn_fc2 = torch.nn.utils.spectral_norm(torch.nn.Linear(128, 3))
        self.down_sample = torch.nn.Conv2d(160, 48, 3, padding=1)


class _SingleLayerNet(torch.nn.Module):
    """models/ITA_single_layer/model.py's parameter tree: attention_block / ffn_block / norm1 / norm2, the unused
    down_sample Conv2d(160, 48, 3), decoder and nn_fc2 under spectral_norm"""

    def __init__(self, E=64, P=192, F=256):
        super().__init__()
        self.tokenizer = Tokenizer(E)
        self.attention_block = Attention(E, P)
        self.ffn_block = Ffn(E, F)
        self.norm1, self.norm2 = torch.nn.LayerNorm(E), torch.nn.LayerNorm(E)
        self.decoder = torch.nn.utils.spectral_norm(torch.nn.Linear(E * 128, 512))
        self.lstm = torch.nn.LSTM(input_size=517, hidden_size=128, num_layers=3)
        self.nn_fc2 = torch.nn.utils.spectral_norm(torch.nn.Linear(128, 3))
        self.down_sample = torch.nn.Conv2d(160, 48, 3, padding=1)


def _checkpoint(E, seed):
    """a float checkpoint in the model file's own state_dict layout, holding synth.float_params(seed, tail=False)"""
    L = GRAPHS[E][1]
    fp = synth.float_params(seed, E=E, num_layers=L, tail=False)
    if E == 128:
        net, ren = _UpsampleShuffleNet(), lambda k: k.replace("norms1.", "norm1_layers.").replace("norms2.", "norm2_layers.")
    else:
        net = _SingleLayerNet()
        ren = lambda k: (k.replace("attention_blocks.0.", "attention_block.").replace("ffn_blocks.0.", "ffn_block.")
                         .replace("norms1.0.", "norm1.").replace("norms2.0.", "norm2."))
    torch.manual_seed(seed)
    src = {ren(k): v for k, v in fp.items()}
    with torch.no_grad():
        for k, v in net.state_dict().items():
            s = k.replace("weight_orig", "weight")
            if s in src and not k.endswith(("weight_u", "weight_v")):
                assert tuple(v.shape) == src[s].shape, k
                v.copy_(torch.from_numpy(src[s]))
    sd = net.state_dict()
    assert "decoder.weight_orig" in sd and "decoder.weight_u" in sd and "decoder.weight" not in sd
    assert tuple(sd["down_sample.weight"].shape) == (48, 160, 3, 3)
    return sd, fp, L


@pytest.mark.parametrize("E", [128, 64])
def test_export_checkpoint_of_each_model_file(tmp_path, E):
    sd, fp, L = _checkpoint(E, 4)
    ck = tmp_path / "model.pth"
    torch.save(sd, str(ck))
    out = tmp_path / "w.itaw"
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "export_blob.py"), "--checkpoint", str(ck),
                        "--out", str(out), "--num-layers", str(L)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    blob = out.read_bytes()
    folded = dict(fp)
    folded["decoder.weight"] = params.fold_spectral_norm(sd, "decoder")
    folded["nn_fc2.weight"] = params.fold_spectral_norm(sd, "nn_fc2")
    assert blob == params.blob_from_float_params(folded, L)
    assert blob == params.blob_from_state_dict(sd, L)
    hdr = np.frombuffer(blob[12:44], np.int32)
    assert int(hdr[0]) == E and int(hdr[6]) == 0
    assert not [k for k in unpack(blob) if k.startswith("tail.")]


def test_decoder_width_decides_the_tail():
    sd, _, _ = _checkpoint(64, 5)
    fp = params.float_params_from_state_dict(sd, 1)
    assert "down_sample.weight" not in fp and fp["decoder.weight"].shape == (512, 8192)
    bad = dict(sd)
    bad["decoder.weight_orig"], bad["decoder.weight_v"] = torch.ones((512, 1000)), torch.ones(1000)
    with pytest.raises(ValueError, match="4608"):
        params.float_params_from_state_dict(bad, 1)
