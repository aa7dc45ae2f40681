"""Long float attention on ragged batches on the MI355X (ita_mha_long_f32_ragged, ita_encoder_layer_long_f32_ragged;
csrc/ita_long_f32_ragged_kernel.h): rows below a frame's length lie within the project's bound (long_f32_common.bound:
max(1e-5, 3 x e_torch)) of float64 on the unpadded frame, whatever the padding holds; with lengths on 64-key unit edges
they carry mha_long_f32's bits.  Cases, inputs (padding: 4 x noise) and references: ragged_f32_cases.py.
Measured on an MI355X, err / e_torch over the valid rows: attention 0.11 .. 1.67, layer 0.23 .. 0.76; the frames of one
token (e_torch about 1e-7, the bound is its floor 1e-5, err 1.3e-7 .. 5.7e-7) 1.04 .. 2.25."""
import numpy as np
import pytest
import torch

from conftest import golden_files
from drone_oa_iree_vit_accelerator_amd import host, params
from gpu_support import INVALID, UNSUPPORTED, Canaries, cu, engine_pool, refused, same_bits
import long_f32_common as lc
from long_cases import long_case, long_f32 as quantiser_safe_tokens
from only_attn_common import fp as only_attn_fp, tensors as only_attn_tensors
from ragged_f32_cases import CASES, case_id, inputs, refs

pytestmark = pytest.mark.gpu

lens_t = lambda lens: torch.tensor(lens, dtype=torch.int32, device="cuda")
MIXED, C200 = CASES[-1], CASES[7]


@pytest.fixture(scope="module")
def engines():
    yield from engine_pool(lambda E: lc.case(E)[1])


def _check(got, lens, ref, what, zeros_behind):
    """every frame: valid rows within the bound of float64 (prints err / e_torch first); rows behind: 0 or finite"""
    for b, (n, (want, e_torch)) in enumerate(zip(lens, ref)):
        g = got[b].cpu().numpy()
        assert (g[n:] == 0).all() if zeros_behind else np.isfinite(g[n:]).all(), (what, b)
        if n:
            assert np.isfinite(g[:n]).all(), (what, b)
            err = float(np.abs(g[:n] - want).max())
            print(f"{what} frame {b} len {n}: |gpu - float64| = {err:.3e}, e_torch = {e_torch:.3e}, ratio {err / e_torch:.2f}")
            assert err <= lc.bound(e_torch), (what, b, err, e_torch)


@pytest.mark.parametrize("rev", [False, True], ids=["ramp", "ramp_rev"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
@pytest.mark.parametrize("E", [64, 128])
def test_definition(engines, E, case, rev):
    x, lt = cu(inputs(E, *case, rev)), lens_t(case[1])
    for l in range(lc.LAYERS[E]):
        _check(engines(E).mha_long_f32_ragged(x, lt, l), case[1], refs("attn", E, *case, rev, l), f"E={E} {case_id(case)} layer {l}", True)


@pytest.mark.parametrize("case", [C200, MIXED], ids=case_id)
@pytest.mark.parametrize("E", [64, 128])
def test_padding_is_invisible(engines, E, case):
    """NaN and +-Inf behind the valid tokens: the same bits as with noise there"""
    x, lt = inputs(E, *case).copy(), lens_t(case[1])
    want = engines(E).mha_long_f32_ragged(cu(x), lt)
    for b, n in enumerate(case[1]):
        x[b, n:] = np.resize(np.array([np.nan, np.inf, -np.inf], np.float32), x[b, n:].shape)
    assert same_bits({"y": engines(E).mha_long_f32_ragged(cu(x), lt)}, {"y": want}, ("y",))


@pytest.mark.parametrize("S_pad", [256, 384])
@pytest.mark.parametrize("E", [64, 128])
def test_bits_of_the_parent(engines, E, S_pad):
    """lens == S_pad (and above: clamped) is mha_long_f32; lengths on unit edges give mha_long_f32 of the unpadded frame"""
    eng, lens = engines(E), (128, 256, 384)
    x = cu(inputs(E, S_pad, (S_pad, S_pad)))
    assert torch.equal(eng.mha_long_f32_ragged(x, lens_t((S_pad, S_pad + 5))), eng.mha_long_f32(x))
    x = cu(inputs(E, 384, lens))
    got = eng.mha_long_f32_ragged(x, lens_t(lens))
    for b, n in enumerate(lens):
        assert torch.equal(got[b, :n], eng.mha_long_f32(x[b:b + 1, :n].contiguous())[0]), (b, n)


@pytest.mark.parametrize("case", [C200, MIXED], ids=case_id)
@pytest.mark.parametrize("E", [64, 128])
def test_layer(engines, E, case):
    """every layer against float64 on the unpadded frames; all rows finite; out aliasing x; encode is the layers chained"""
    eng, (S_pad, lens) = engines(E), case
    x, lt = cu(inputs(E, *case)), lens_t(lens)
    chained = x
    for l in range(lc.LAYERS[E]):
        got = eng.encoder_layer_long_f32_ragged(x, lt, l)
        _check(got, lens, refs("layer", E, *case, False, l), f"layer E={E} {case_id(case)} layer {l}", False)
        alias = x.clone()
        assert eng.encoder_layer_long_f32_ragged(alias, lt, l, out=alias) is alias and torch.equal(alias, got), f"layer {l} in place"
        chained = eng.encoder_layer_long_f32_ragged(chained, lt, l)
    assert torch.equal(eng.encode_long_f32_ragged(x, lt), chained)


@pytest.mark.parametrize("case", [C200, MIXED], ids=case_id)
def test_layer_only_attn_equals_oracle(oracle, case):
    """ITAW0002 (int8 ragged attention, float FFN): valid rows are the oracle composition of test_gpu_long_f32.py on the
    unpadded frame, bit for bit"""
    S_pad, lens = case
    d = params.load_fixture(golden_files("onlyattn1l_E64_s0_B2.npz")[0])
    fp = only_attn_fp(d)
    t, eng = only_attn_tensors(d, fp), host.Engine(params.blob_from_record(d, fp, E=64, num_layers=1), device=0)
    x = quantiser_safe_tokens(S_pad + len(lens), len(lens), S_pad, 64, t, 0)
    got = eng.encoder_layer_long_f32_ragged(cu(x), lens_t(lens))
    assert bool(torch.isfinite(got).all())
    for b, n in enumerate(lens):
        if n:
            xb = x[b:b + 1, :n]
            x1 = oracle.add_ln(xb, oracle.mha(xb, t, 0), t["norm1_0.w"], t["norm1_0.b"])
            hid = np.maximum(oracle.linear_f32(x1, t["ffn0.w1f"], t["ffn0.b1f"]), np.float32(0))
            want = oracle.add_ln(x1, oracle.linear_f32(hid, t["ffn0.w2f"], t["ffn0.b2f"]), t["norm2_0.w"], t["norm2_0.b"])
            np.testing.assert_array_equal(got[b, :n].cpu().numpy(), want[0], err_msg=f"frame {b}")
    eng.close()


@pytest.mark.parametrize("E", [64, 128])
def test_capture_follows_new_lengths(engines, E):
    """one captured call (gpu_support's protocol: a call before the capture, several replays against the eager result,
    canaries behind the output) follows the lengths that lie in device memory at each replay"""
    eng, (S_pad, lens) = engines(E), MIXED
    x, lt = cu(inputs(E, S_pad, lens)), lens_t(lens)
    c = Canaries({"y": (tuple(x.shape), torch.float32)})
    eng.mha_long_f32_ragged(x, lt)      # the workspace has its size before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        host._chk(host.lib().ita_mha_long_f32_ragged(eng._h, 0, x.data_ptr(), c.ptr("y"), len(lens), S_pad, lt.data_ptr(),
                                                     host._stream_ptr(0)))
    for replay, now in enumerate((lens, lens, (5, 384, 130, 256, 0, 64), lens)):
        lt.copy_(lens_t(now))
        g.replay()
        torch.cuda.synchronize()
        assert same_bits(c.views(), {"y": eng.mha_long_f32_ragged(x, lens_t(now))}, ("y",)), (replay, now)
        c.assert_untouched(written=("y",))
        c.refill()
    del g


def test_refusals(engines):
    """refused before any launch, outputs untouched; the handle runs on"""
    E, (S_pad, lens) = 64, C200
    x, lt = cu(inputs(E, S_pad, lens)), lens_t(lens)
    c = Canaries({"y": ((1, S_pad, E), torch.float32)})
    L = host.lib()
    mha = lambda e, S=S_pad, lp=lt.data_ptr(): host._chk(L.ita_mha_long_f32_ragged(e._h, 0, x.data_ptr(), c.ptr("y"), 1, S, lp, host._stream_ptr(0)))
    layer = lambda e, S=S_pad, lp=lt.data_ptr(): host._chk(L.ita_encoder_layer_long_f32_ragged(e._h, 0, x.data_ptr(), c.ptr("y"), 1, S, lp, host._stream_ptr(0)))
    e1, e2 = (host.Engine(long_case(f).blob, device=0) for f in ("vitlstm_E64_seed0_B2", "onlyattn1l_E64_s0_B2"))   # ITAW0001, ITAW0002
    for e, entry, names in ((e1, mha, "ita_mha_long_int8_ragged"), (e2, mha, "ita_mha_long_int8_ragged"), (e1, layer, "ita_encoder_layer_long_ragged")):
        refused(lambda: entry(e), c, UNSUPPORTED)
        assert names in L.ita_error_string().decode()
    e1.close(); e2.close()
    eng = engines(E)
    for entry in (mha, layer):
        for S in (200, 0):
            refused(lambda: entry(eng, S=S), c, UNSUPPORTED)
        for lp in (None, lt.data_ptr() + 2):
            refused(lambda: entry(eng, lp=lp), c, INVALID)
    for bad in (lt.long(), lens_t((200, 200)), lt.cpu()):
        for call in (eng.mha_long_f32_ragged, eng.encoder_layer_long_f32_ragged, eng.encode_long_f32_ragged):
            with pytest.raises(host.ITAError, match="lens must be"):
                call(x, bad)
    _check(eng.mha_long_f32_ragged(x, lt), lens, refs("attn", E, S_pad, lens), "after refusals", True)
