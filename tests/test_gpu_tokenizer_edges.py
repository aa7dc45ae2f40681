"""The tokenizer kernels on crafted per-channel scales and 0 / 255 frames (tokenizer_edges_common): every stock E = 64 blob has
one exponent e_c for all channels and the stock frames never hold pixel code 255, so a table that mixed the channels' scales,
or a window that let a neighbour's bytes in, would pass the stock tests.

Routes, each bit-equal to oracle.tokenizer and therefore inside the 1e-5 float64 bound (both asserted, so an error shared by
oracle and kernel is named too; tests/test_tokenizer_edges_cpu.py holds the oracle to an independent model and to float64):
    ita_tok_stream_kernel<E, true>   Engine-level ita_tokenizer on u8 frames, E = 64 and 128
    ita_tok_stream_kernel<E, false>  ita_tokenizer on f32 frames, E = 64 and 128
    ita_stream_kernel<64, true, 1>   ita_vitlstm_forward's tokens / x1 / x2 taps on u8 frames, layer_forms()["tok_image"] asserted
Every output is written into canary buffers (the pad behind it stays untouched) and every call runs twice with equal bits."""
import ctypes

import numpy as np
import pytest

import tokenizer_edges_common as tc
from conftest import golden_files
from drone_oa_iree_vit_accelerator_amd import host, params, synth
from gpu_support import Canaries, cu, engine_pool

pytestmark = pytest.mark.gpu

NF = len(tc.FRAME_NAMES)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


_BLOBS = {}


def _blob(E, name):
    """the stock record of E with the four tokenizer.* float parameters replaced by the set's"""
    if (E, name) not in _BLOBS:
        cw, cb, lw, lb = tc.weights(E, name)
        if E == 64:
            d = params.load_fixture(golden_files("vitlstm_E64_seed0_B2.npz")[0])
            fp, kw = synth.float_params(0, E=64), {}
        else:
            d = params.load_fixture(golden_files("vit2l_E128_s0_B2.npz")[0])
            nl = int(d["meta.num_layers"])
            fp, kw = synth.float_params(int(d["meta.seed"]), E=128, num_layers=nl, tail=False), dict(num_layers=nl)
        fp = dict(fp)
        fp.update({"tokenizer.conv.weight": cw.reshape(E, 1, 7, 7).copy(), "tokenizer.conv.bias": cb.copy(),
                   "tokenizer.norm.weight": lw.copy(), "tokenizer.norm.bias": lb.copy()})
        _BLOBS[E, name] = params.blob_from_record(d, fp, E=E, **kw)
    return _BLOBS[E, name]


@pytest.fixture(scope="module")
def engines():
    yield from engine_pool(_blob)


def _frames(dtype, idx=slice(None)):
    f = tc.frames()[idx]
    return f if dtype == "u8" else tc.frames_f32(f)


_WANT = {}


def _want(oracle, E, name, dtype):
    """oracle.tokenizer of every frame, once per (E, set, frame type)"""
    if (E, name, dtype) not in _WANT:
        _WANT[E, name, dtype] = oracle.tokenizer(_frames(dtype), *tc.weights(E, name))
        _WANT[E, name, dtype].setflags(write=False)
    return _WANT[E, name, dtype]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _twice(torch, call, can, names):
    """call() writes the canaries' outputs `names`: run twice, same bits, nothing else written -> {name: numpy array}"""
    runs = []
    for _ in range(2):
        can.refill()
        rc = call()
        torch.cuda.synchronize()
        assert rc == 0, host.lib().ita_error_string(rc)
        can.assert_untouched(written=names)
        runs.append({k: v.cpu().numpy() for k, v in can.views().items() if k in names})
    for k in names:
        assert np.array_equal(_bits(runs[0][k]), _bits(runs[1][k])), f"{k}: two runs of one call differ"
    return runs[0]


def _tokenize(torch, eng, img):
    """ita_tokenizer into a canary buffer, twice -> tokens (B, 128, E)"""
    x = cu(img)
    B = x.shape[0]
    can = Canaries({"tokens": ((B, 128, eng.E), torch.float32)})
    dt = host.IMAGE_U8 if x.dtype == torch.uint8 else host.IMAGE_F32
    call = lambda: host.lib().ita_tokenizer(eng._h, x.data_ptr(), dt, can.ptr("tokens"), B, host._stream_ptr(eng.device))
    return _twice(torch, call, can, ("tokens",))["tokens"]


FWD = ("tokens", "x1", "x2", "vel", "h", "c")


def _inputs(B):
    fr = synth.frames(0, NF)
    i = np.arange(B) % NF
    return fr["desvel"][i].reshape(B), fr["quat"][i]


def _forward(torch, eng, img):
    """ita_vitlstm_forward on u8 frames with the tokens / x1 / x2 taps, every output a canary buffer, twice"""
    x = cu(img)
    B = x.shape[0]
    dv, qt = (cu(a) for a in _inputs(B))
    zero = torch.zeros((3, B, 128), dtype=torch.float32, device=x.device)
    tok = ((B, 128, eng.E), torch.float32)
    can = Canaries(dict(tokens=tok, x1=tok, x2=tok, vel=((B, 3), torch.float32), h=((3, B, 128), torch.float32),
                        c=((3, B, 128), torch.float32)))
    st = host._FwdTaps(tokens=can.ptr("tokens"), x1=can.ptr("x1"), x2=can.ptr("x2"), feat=None, dec=None)
    call = lambda: host.lib().ita_vitlstm_forward(eng._h, x.data_ptr(), host.IMAGE_U8, dv.data_ptr(), qt.data_ptr(),
                                                  zero.data_ptr(), zero.data_ptr(), can.ptr("vel"), can.ptr("h"), can.ptr("c"),
                                                  B, ctypes.byref(st), host._stream_ptr(eng.device))
    return _twice(torch, call, can, FWD)


def _oracle_forward(oracle, name, idx):
    img = tc.frames()[idx % NF]
    dv, qt = _inputs(int(idx.max()) + 1)
    return oracle.forward(_blob(64, name), img, dv[idx], qt[idx], taps=True)[3]


def _check_tokens(got, want, E, name, what):
    """bit equality with the oracle, the float64 bound, and the one-hot frames' footprints (got: every frame of tc.frames)"""
    err = float(np.abs(got - tc.tokens_f64_of(E, name)).max())
    print(f"{what} E = {E} {name}: max |tokens - f64| = {err:.2e}")
    bad = [tc.FRAME_NAMES[i] for i in range(NF) if not np.array_equal(_bits(got[i]), _bits(want[i]))]
    assert not bad, f"{what} E = {E} {name}: differs from the oracle on frames {bad}"
    assert err <= tc.BOUND
    g = _bits(got)
    for i, (r, c) in enumerate(tc.ONE_HOT):
        out = ~tc.footprint(r, c)
        assert np.array_equal(g[tc.FIRST_HOT + i][out], g[tc.ZEROS][out]), f"{what}: pixel {(r, c)} moved a token outside its footprint"


@pytest.mark.parametrize("dtype", ["u8", "f32"])
@pytest.mark.parametrize("name", tc.SETS)
@pytest.mark.parametrize("E", tc.ES)
def test_standalone_kernel_every_set_and_frame(torch_cuda, oracle, engines, E, name, dtype):
    """ita_tok_stream_kernel<E, U8>: ita_tokenizer on every frame of every set"""
    got = _tokenize(torch_cuda, engines(E, name), _frames(dtype))
    _check_tokens(got, _want(oracle, E, name, dtype), E, name, f"ita_tokenizer {dtype}")


@pytest.mark.parametrize("name", tc.SETS)
def test_fused_kernel_every_set_and_frame(torch_cuda, oracle, engines, name):
    """the tokenizer inside ita_stream_kernel<64, true, 1>: the forward's tokens, x1 and x2 on every frame of every set"""
    eng = engines(64, name)
    assert eng.layer_forms()["tok_image"], "the blob lost its fused-tokenizer image: the forward would run the split route"
    got = _forward(torch_cuda, eng, tc.frames())
    want = _oracle_forward(oracle, name, np.arange(NF))
    _check_tokens(got["tokens"], want["tokens"], 64, name, "fused forward")
    assert np.array_equal(_bits(want["tokens"]), _bits(_want(oracle, 64, name, "u8")))
    for k in ("x1", "x2"):
        assert np.array_equal(_bits(got[k]), _bits(want[k])), f"fused forward {name}: {k} differs from the oracle"
    alone = _tokenize(torch_cuda, eng, tc.frames())
    assert np.array_equal(_bits(got["tokens"]), _bits(alone)), "fused and stand-alone tokens differ"


ROUTES = [(64, "u8"), (64, "f32"), (128, "u8"), (128, "f32"), (64, "fused")]


@pytest.mark.parametrize("E,route", ROUTES, ids=lambda v: str(v))
def test_frames_do_not_leak_into_their_neighbours(torch_cuda, engines, E, route):
    """[0, 255, 0] and [255, 0, 255]: every frame's tokens have the bits of the same frame run alone -- the dwords a window
    fetches past byte 5399 and before byte 0 of its frame belong to the neighbour"""
    eng = engines(E, "graded")
    if route == "fused":
        assert eng.layer_forms()["tok_image"]
        run = lambda idx: _forward(torch_cuda, eng, tc.frames()[idx])["tokens"]
    else:
        run = lambda idx: _tokenize(torch_cuda, eng, _frames(route, idx))
    alone = {i: run([i])[0] for i in (tc.ZEROS, tc.FULL)}
    assert not np.array_equal(_bits(alone[tc.ZEROS]), _bits(alone[tc.FULL]))
    for batch in ([tc.ZEROS, tc.FULL, tc.ZEROS], [tc.FULL, tc.ZEROS, tc.FULL]):
        got = run(batch)
        for j, i in enumerate(batch):
            assert np.array_equal(_bits(got[j]), _bits(alone[i])), f"frame {j} of {[tc.FRAME_NAMES[i] for i in batch]}"


@pytest.mark.parametrize("E,route", [(64, "u8"), (128, "u8"), (64, "fused")], ids=lambda v: str(v))
def test_past_one_frame_per_workgroup_with_crafted_tables(torch_cuda, oracle, engines, E, route):
    """`graded` where a workgroup takes a second frame (stand-alone: 2 CUs + 3 frames on 2 CUs workgroups; fused: CUs + 2
    on CUs), frames cycled from the list: both ends and the two frames around the wrap against the oracle"""
    cus = torch_cuda.cuda.get_device_properties(0).multi_processor_count
    eng = engines(E, "graded")
    if route == "fused":
        assert eng.layer_forms()["tok_image"]
        B = cus + 2
        sel = np.array([0, cus - 1, cus, B - 1])
        got = _forward(torch_cuda, eng, tc.frames()[np.arange(B) % NF])
        want = _oracle_forward(oracle, "graded", sel)
        keys = ("tokens", "x1", "x2")
    else:
        B = 2 * cus + 3
        sel = np.array([0, 2 * cus - 1, 2 * cus, B - 1])
        got = {"tokens": _tokenize(torch_cuda, eng, tc.frames()[np.arange(B) % NF])}
        want = {"tokens": _want(oracle, E, "graded", "u8")[sel % NF]}
        keys = ("tokens",)
    for k in keys:
        assert np.array_equal(_bits(got[k][sel]), _bits(want[k])), f"{route} E = {E}, B = {B}: {k} differs on frames {sel}"
    assert float(np.abs(got["tokens"][sel] - tc.tokens_f64_of(E, "graded")[sel % NF]).max()) <= tc.BOUND
