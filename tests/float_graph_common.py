"""The ITAW blob's unpacker and repacker, the built plugin's validator and the float model's parameter tree, shared by
the CPU and the GPU tests of the float graph.  CPU only."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import golden_files
from drone_oa_iree_vit_accelerator_amd import params, synth

_NP = {0: np.float32, 1: np.int8, 2: np.int32, 3: np.uint8, 4: np.float16}


def unpack(blob):
    n = np.frombuffer(blob[8:12], np.int32)[0]
    t = {}
    for i in range(n):
        e = blob[64 + 72 * i: 64 + 72 * (i + 1)]
        nm = e[:32].split(b"\0")[0].decode()
        dt, nd = np.frombuffer(e[32:40], np.int32)
        shape = [int(s) for s in np.frombuffer(e[40:56], np.int32)[:nd]]
        off, nb = (int(v) for v in np.frombuffer(e[56:72], np.int64))
        t[nm] = np.frombuffer(blob[off:off + nb], _NP[int(dt)]).reshape(shape).copy()
    return t


def repack(blob, t, magic=None):
    hdr = np.frombuffer(blob[12:44], np.int32)
    E, S, P, F, H, L, has_tail = (int(v) for v in hdr[:7])
    magic = magic or blob[:8]
    return params.pack_blob(t, E=E, S=S, P=P, F=F, H=H, num_layers=L, has_tail=bool(has_tail),
                            ffn_f32=magic != b"ITAW0001", attn_f32=magic == b"ITAW0003")


@pytest.fixture(scope="module")
def plugin():
    from drone_oa_iree_vit_accelerator_amd import host
    so = host.build_extension()
    lib = C.CDLL(so)
    lib.ita_validate_blob.argtypes = [C.c_void_p, C.c_size_t, C.c_char_p]
    return lib


def validate(lib, blob):
    bad = C.create_string_buffer(32)
    buf = C.create_string_buffer(blob, len(blob))
    rc = lib.ita_validate_blob(buf, len(blob), bad)
    return rc, bad.value.decode()


class Attention(torch.nn.Module):
    def __init__(self, E, P):
        super().__init__()
        self.q_proj, self.k_proj = torch.nn.Linear(E, P), torch.nn.Linear(E, P)
        self.v_proj, self.out_proj = torch.nn.Linear(E, P), torch.nn.Linear(P, E)


class Ffn(torch.nn.Module):
    def __init__(self, E, F):
        super().__init__()
        self.fc1, self.fc2 = torch.nn.Linear(E, F), torch.nn.Linear(F, E)


class Tokenizer(torch.nn.Module):
    def __init__(self, E):
        super().__init__()
        self.conv = torch.nn.Conv2d(1, E, 7, stride=2, padding=3)
        self.norm = torch.nn.LayerNorm(E)


class FloatNet(torch.nn.Module):
    """the float model's parameter tree under its state_dict names (models/ITA_single_layer_upsample_shuffle/model.py),
    decoder and nn_fc2 under spectral_norm as declared there"""

    def __init__(self, L, E=64, P=192, F=256):
        super().__init__()
        self.tokenizer = Tokenizer(E)
        self.attention_blocks = torch.nn.ModuleList(Attention(E, P) for _ in range(L))
        self.ffn_blocks = torch.nn.ModuleList(Ffn(E, F) for _ in range(L))
        self.norms1 = torch.nn.ModuleList(torch.nn.LayerNorm(E) for _ in range(L))
        self.norms2 = torch.nn.ModuleList(torch.nn.LayerNorm(E) for _ in range(L))
        self.down_sample = torch.nn.Conv2d(E // 4 + E, 9, 3, padding=1)
        self.decoder = torch.nn.utils.spectral_norm(torch.nn.Linear(4608, 512))
        self.lstm = torch.nn.LSTM(input_size=517, hidden_size=128, num_layers=3)
        self.nn_fc2 = torch.nn.utils.spectral_norm(torch.nn.Linear(128, 3))


def float_state_dict(L, seed):
    fp = synth.float_params(seed, E=64, num_layers=L)
    torch.manual_seed(seed)
    net = FloatNet(L)
    with torch.no_grad():
        for k, v in net.state_dict().items():
            src = k.replace("weight_orig", "weight")
            if src in fp and not k.endswith(("weight_u", "weight_v")):
                assert tuple(v.shape) == fp[src].shape, k
                v.copy_(torch.from_numpy(fp[src]))
    sd = net.state_dict()
    assert "decoder.weight_orig" in sd and "decoder.weight_u" in sd and "decoder.weight" not in sd
    assert "attention_blocks.0.q_proj.weight" in sd
    return sd


FLOAT_FIX = {1: golden_files("floattwin_E64_s0_B2.npz")[0], 2: golden_files("floattwin2l_E64_s1_B2.npz")[0]}


def setup_float(L):
    d = params.load_fixture(FLOAT_FIX[L])
    fp = synth.float_params(int(d["meta.seed"]), E=64, num_layers=L)
    assert str(d["meta.params_sha256"]) == synth.digest(fp)
    return d, fp, params.blob_from_float_params(fp, L)


NOTAIL_GRAPHS = {128: ("floatnt2l_E128_s1_B2.npz", 2), 64: ("floatnt1l_E64_s2_B2.npz", 1)}


def setup_notail(E):
    name, L = NOTAIL_GRAPHS[E]
    d = params.load_fixture(golden_files(name)[0])
    fp = synth.float_params(int(d["meta.seed"]), E=E, num_layers=L, tail=False)
    assert str(d["meta.params_sha256"]) == synth.digest(fp)
    return d, fp, params.blob_from_float_params(fp, L), L


def ln_like(B, seed, E):
    """LayerNorm-like activations: per token zero mean, unit variance, then a mild affine"""
    rs = np.random.RandomState(seed)
    x = rs.standard_normal((B, 128, E))
    x = (x - x.mean(-1, keepdims=True)) / x.std(-1, keepdims=True)
    return (x * (1.0 + 0.1 * rs.standard_normal(E)) + 0.1 * rs.standard_normal(E)).astype(np.float32)


def attn64(x, fp, i):
    """ITASelfAttention.forward (models/ITA/layers.py:67-88) in float64: one head, no 1/sqrt(d)"""
    g = lambda k: fp[f"attention_blocks.{i}.{k}"].astype(np.float64)
    x = x.astype(np.float64)
    q, k, v = (x @ g(f"{n}.weight").T + g(f"{n}.bias") for n in ("q_proj", "k_proj", "v_proj"))
    s = q @ k.transpose(0, 2, 1)
    p = np.exp(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    return (p @ v) @ g("out_proj.weight").T + g("out_proj.bias")


def converted_state_dict(path):
    """the reference's converted state_dict as tools/gen_golden.py (gen_checkpoint) recorded it: key order, packed
    quantized Linears, observer scales; the unchanged float parameters are the fixture seed's synthetic ones"""
    d = np.load(path)
    fp = synth.float_params(int(d["meta.seed"]), E=64)
    assert str(d["meta.params_sha256"]) == synth.digest(fp)
    sd = {}
    for k in d["keys"]:
        k = str(k)
        if "d." + k in d:
            sd[k] = getattr(torch, str(d["d." + k]))
        elif "q." + k + ".int_repr" in d:
            w = torch._make_per_tensor_quantized_tensor(torch.from_numpy(d["q." + k + ".int_repr"]),
                                                        float(d["q." + k + ".scale"]), int(d["q." + k + ".zero_point"]))
            sd[k] = (w, torch.from_numpy(d["q." + k + ".bias"]))
        elif "t." + k in d:
            sd[k] = torch.from_numpy(d["t." + k])
        else:
            sd[k] = torch.from_numpy(fp[k])
    return sd
