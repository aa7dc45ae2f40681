"""Long-sequence encoder layers on the MI355X: ita_mha_long_q8 at E = 64, ita_mha_long_int8 (Engine.mha_long) and
ita_encoder_layer_long (Engine.encoder_layer_long / encode_long) at E = 64 and E = 128, bit for bit against the oracle
composition  a = mha(x);  x1 = add_ln(x, a, norm1);  x2 = add_ln(x1, ffn(x1), norm2)  (equality for int
tensors, x1 and x2).

Shapes (S, B): (128, 3) one key tile, the ring prefetch wraps onto tile 0; (256, 2) / (384, 2) even and odd tile counts,
so the ring-slot parity differs across the three sweeps; B > 1 the frame strides of the workspace; (1024, 1) a longer row
sum; one S = 8192 case on sampled rows.

Which requantisation form (FAST: all six sites pass the load-time single-rounding proof; exact otherwise) each fixture
selects, i.e. which instantiation of ita_long_proj_kernel / ita_long_attn_kernel<FAST, E, io> it runs:
    E = 64   blocks_E64_seed2_B1   exact      vitlstm_E64_seed0_B2  FAST      vitlstm_E64_seed1_B2, _seed2_B2  exact
    E = 128  blocks_E128_seed0_B1  exact (site O fails)     blocks_E128_seed1_B1  exact (site Q fails)
             vit2l_E128_s0_B2      exact, both layers       vit2l_us_E128_s1_B2   FAST, both layers
test_long_f32_quantiser_edges gives the f32 entries ties, saturating and zero tokens on the FAST and the exact one of each E;
so both forms run at both E, in the int8 form (E = 128 exact: tests/test_gpu_parity.py; E = 128 FAST: vit2l_us here) and
in the f32 form."""
import numpy as np
import pytest

from conftest import golden_files
from drone_oa_iree_vit_accelerator_amd import host, params, synth
from heads_common import FIX_HEADS_2L, case as heads_case
from gpu_support import UNSUPPORTED, Canaries, cu, refused
from long_cases import long_case, long_f32, long_inputs
from only_attn_common import fp as only_attn_fp

pytestmark = pytest.mark.gpu

SHAPES = [(128, 3), (256, 2), (384, 2), (1024, 1)]
E64_BLOCKS, E64_VIT = "blocks_E64_seed2_B1", ["vitlstm_E64_seed0_B2", "vitlstm_E64_seed1_B2", "vitlstm_E64_seed2_B2"]
E128_BLOCKS, E128_VIT, E128_FAST = ["blocks_E128_seed0_B1", "blocks_E128_seed1_B1"], "vit2l_E128_s0_B2", "vit2l_us_E128_s1_B2"


def _layer(oracle, x, t, fp, l):
    a = oracle.mha(x, t, l)
    x1 = oracle.add_ln(x, a, fp[f"norms1.{l}.weight"], fp[f"norms1.{l}.bias"])
    return oracle.add_ln(x1, oracle.ffn(x1, t, l), fp[f"norms2.{l}.weight"], fp[f"norms2.{l}.bias"])


@pytest.mark.parametrize("S,B", SHAPES)
def test_mha_long_q8_e64_equals_oracle(oracle, S, B):
    """ita_long_*_kernel<FAST | exact, 64, int8>: the whole output against oracle.mha_q8; at S = 128 also ita_mha_q8"""
    for name in (E64_BLOCKS, E64_VIT[0], E64_VIT[1]):
        case = long_case(name)
        E, t, blob = case.E, case.t, case.blob
        eng = host.Engine(blob, device=0)
        xq = long_inputs(S + B, B, S, E)
        got = eng.mha_long_q8(cu(xq)).cpu().numpy()
        want = oracle.mha_q8(xq, t)
        np.testing.assert_array_equal(got, want, err_msg=name)
        assert len({r.tobytes() for r in got[0]}) > S // 4, name
        if S == 128:
            np.testing.assert_array_equal(eng.mha_q8(cu(xq)).cpu().numpy(), want, err_msg=name)
        eng.close()


@pytest.mark.parametrize("S,B", [(128, 3), (384, 2)])
def test_mha_long_q8_e128_fast_form(oracle, S, B):
    """ita_long_*_kernel<FAST, 128, int8>, which no blocks_E128 fixture selects: both layers of vit2l_us_E128_s1"""
    case = long_case(E128_FAST)
    E, nl, t, blob = case.E, case.num_layers, case.t, case.blob
    eng = host.Engine(blob, device=0)
    xq = long_inputs(S + B, B, S, E)
    for l in range(nl):
        np.testing.assert_array_equal(eng.mha_long_q8(cu(xq), l).cpu().numpy(), oracle.mha_q8(xq, t, l), err_msg=f"layer {l}")
    eng.close()


def test_mha_long_q8_e64_config5_size(oracle):
    """S = 8192 at E = 64: 16 sampled rows against oracle.mha_q8_rows, two runs bit-identical"""
    import torch
    case = long_case(E64_VIT[0])
    E, t, blob = case.E, case.t, case.blob
    eng = host.Engine(blob, device=0)
    S = 8192
    xq = long_inputs(99, 1, S, E)
    x = cu(xq)
    a1, a2 = eng.mha_long_q8(x), eng.mha_long_q8(x)
    assert torch.equal(a1, a2)
    rows = [0, 1, 127, 128, 129, 1000, 2047, 2048, 4095, 4096, 5000, 6143, 7000, 8063, 8064, 8191]
    got = a1.cpu().numpy()[0]
    np.testing.assert_array_equal(got[rows], oracle.mha_q8_rows(xq[0], t, rows))
    assert len({r.tobytes() for r in got[::64]}) > 32
    eng.close()


@pytest.mark.parametrize("S,B", SHAPES)
@pytest.mark.parametrize("E", [64, 128])
def test_mha_long_f32_equals_oracle(oracle, E, S, B):
    """Engine.mha_long (f32 in, dequantised out_proj out) against oracle.mha; two runs bit-identical, a frame does not
    depend on its batch position"""
    import torch
    names = (E64_BLOCKS, E64_VIT[0]) if E == 64 else (*E128_BLOCKS, E128_FAST)
    for name in names:
        case = long_case(name)
        t, blob = case.t, case.blob
        eng = host.Engine(blob, device=0)
        x = long_f32(S + B, B, S, E, t)
        xc = cu(x)
        got = eng.mha_long(xc)
        np.testing.assert_array_equal(got.cpu().numpy(), oracle.mha(x, t), err_msg=name)
        assert torch.equal(got, eng.mha_long(xc)), name
        assert torch.equal(eng.mha_long(xc.flip(0).contiguous()).flip(0), got), name
        if S == 128:
            np.testing.assert_array_equal(eng.mha(xc).cpu().numpy(), got.cpu().numpy(), err_msg=name)
        eng.close()


@pytest.mark.parametrize("S,B", SHAPES)
@pytest.mark.parametrize("E", [64, 128])
def test_encoder_layer_long_equals_oracle(oracle, E, S, B):
    """Engine.encoder_layer_long against the oracle composition, for every layer of the fixture; at S = 128 also against
    encoder_layer; with out aliasing x; two runs bit-identical; a frame does not depend on its batch position"""
    import torch
    for name in (E64_VIT if E == 64 else [E128_VIT]):
        case = long_case(name)
        nl, t, fp, blob = case.num_layers, case.t, case.fp, case.blob
        eng = host.Engine(blob, device=0)
        for l in range(nl):
            x = long_f32(S + B + l, B, S, E, t, l)
            xc = cu(x)
            got = eng.encoder_layer_long(xc, l)
            np.testing.assert_array_equal(got.cpu().numpy(), _layer(oracle, x, t, fp, l), err_msg=f"{name} layer {l}")
            assert torch.equal(got, eng.encoder_layer_long(xc, l)), name
            assert torch.equal(eng.encoder_layer_long(xc.flip(0).contiguous(), l).flip(0), got), name
            if S == 128:
                assert torch.equal(eng.encoder_layer(xc, l), got), name
            alias = xc.clone()
            assert eng.encoder_layer_long(alias, l, out=alias) is alias
            assert torch.equal(alias, got), f"{name} layer {l}: out aliasing x"
        eng.close()


QUANT_EDGES = [(E64_VIT[0], True), (E64_VIT[1], False), (E128_VIT, False), (E128_FAST, True)]


@pytest.mark.parametrize("name,fast", QUANT_EDGES)
def test_long_f32_quantiser_edges(oracle, name, fast):
    """the long kernels' f32 input at the quantiser's edges, which long_f32's offsets of (-0.4, 0.4) never reach: zero
    tokens, saturating +-50 tokens, a 1e30 token, exact ties 0.5 s and 1.5 s (to even: 0 and 2), a token scaled by 30, among
    ordinary ones at S = 256; mha_long, encoder_layer_long and the statistics against the oracle composition, on the FAST
    and on the exact fixture of each E"""
    from drone_oa_iree_vit_accelerator_amd import attention_stats_ref as asr
    case = long_case(name)
    E, t, fp, blob = case.E, case.t, case.fp, case.blob
    eng = host.Engine(blob, device=0)
    forms = eng.layer_forms(0)
    assert forms["fast"] == fast and forms["attn_image"], (name, forms)
    S, B = 256, 2
    x = long_f32(S + B, B, S, E, t)
    s = np.float32(float(params.load_fixture(golden_files(name + ".npz")[0])["attn0.quant.scale"]))
    x[0, 0:3], x[0, 3:6], x[0, 6:9] = 0.0, 50.0, -50.0
    x[0, 130] = 1e30
    x[0, 140], x[0, 141] = np.float32(0.5) * s, np.float32(1.5) * s
    x[0, 150] *= 30.0
    x[1, 127:129], x[1, 200], x[1, 201] = 0.0, -50.0, np.float32(1.5) * s
    x[1, 255, ::2] *= 30.0
    oy, otaps = oracle.mha(x, t, taps=True)
    xq = otaps["x_q"]
    assert (xq[0, 140] == 0).all() and (xq[0, 141] == 2).all() and (xq[1, 201] == 2).all()      # ties to even
    assert (xq[0, 130] == 127).all() and (xq[0, 3:6] == 127).all() and (xq[0, 6:9] == -128).all() and (xq[0, 0:3] == 0).all()
    assert (np.abs(xq[0, 150].astype(np.int32)) >= 127).sum() > E // 2
    xc = cu(x)
    np.testing.assert_array_equal(eng.mha_long(xc).cpu().numpy(), oy, err_msg=name)
    np.testing.assert_array_equal(eng.mha_long_q8(cu(xq)).cpu().numpy(), otaps["out_q"], err_msg=name)
    want = _layer(oracle, x, t, fp, 0)
    got = eng.encoder_layer_long(xc, 0).cpu().numpy()
    print(f"{name}: the 1e30 token's row: oracle {want[0, 130, :4]}, engine {got[0, 130, :4]}")
    np.testing.assert_array_equal(got, want, err_msg=name)
    st = eng.attention_stats_long(xc)
    for k, v in asr.stats(x, t).items():
        np.testing.assert_array_equal(st[k].cpu().numpy(), v, err_msg=f"{name} statistic {k}")
    eng.close()


def test_encode_long_is_the_layers_chained(oracle):
    """the two-layer E = 128 blob: encode_long equals layer 0 then layer 1, and the oracle's chain"""
    import torch
    case = long_case(E128_VIT)
    E, nl, t, fp, blob = case.E, case.num_layers, case.t, case.fp, case.blob
    assert nl == 2
    eng = host.Engine(blob, device=0)
    S, B = 384, 2
    x = long_f32(7, B, S, E, t)
    xc = cu(x)
    keep = xc.clone()
    got = eng.encode_long(xc)
    assert torch.equal(xc, keep), "encode_long changed its input"
    assert torch.equal(got, eng.encoder_layer_long(eng.encoder_layer_long(xc, 0), 1))
    np.testing.assert_array_equal(got.cpu().numpy(), _layer(oracle, _layer(oracle, x, t, fp, 0), t, fp, 1))
    eng.close()


def _refused(eng, call):
    """call(x, out) must raise ITAError UNSUPPORTED and leave the canary-filled output untouched"""
    import torch
    x = torch.zeros((1, 256, eng.E), dtype=torch.float32, device="cuda")
    c = Canaries({"out": (x.shape, torch.float32)})
    refused(lambda: call(x, c.views()["out"]), c, UNSUPPORTED)


def _mha_long_into(eng):
    def call(x, out):
        host._chk(host.lib().ita_mha_long_int8(eng._h, 0, x.data_ptr(), out.data_ptr(), x.shape[0], x.shape[1],
                                              host._stream_ptr(eng.device)))
    return call


def test_refusals_before_any_launch(oracle):
    """a float-attention blob, an ITAW0002 blob (encoder_layer_long only) and the E = 128, H = 4 blob: UNSUPPORTED, output
    untouched; the handle of the ITAW0002 blob then still runs mha_long_q8 and mha_long correctly"""
    fpf = synth.float_params(1, E=128, num_layers=2, tail=False)
    ef = host.Engine(params.blob_from_float_params(fpf, 2), device=0)
    _refused(ef, _mha_long_into(ef))
    _refused(ef, lambda x, out: ef.encoder_layer_long(x, 0, out=out))
    ef.close()

    _, H, E, nl, _, _, hblob = heads_case(FIX_HEADS_2L[0])
    assert (H, E) == (4, 128)
    eh = host.Engine(hblob, device=0)
    _refused(eh, _mha_long_into(eh))
    _refused(eh, lambda x, out: eh.encoder_layer_long(x, 0, out=out))
    eh.close()

    d = params.load_fixture(golden_files("onlyattn1l_E64_s0_B2.npz")[0])
    eo = host.Engine(params.blob_from_record(d, only_attn_fp(d), E=64, num_layers=1), device=0)
    assert eo.ffn_kind(0) == host.FFN_F32
    _refused(eo, lambda x, out: eo.encoder_layer_long(x, 0, out=out))
    t = params.attention_tensors(d, "attn0.", 0)
    xq = long_inputs(5, 2, 256, 64)
    np.testing.assert_array_equal(eo.mha_long_q8(cu(xq)).cpu().numpy(), oracle.mha_q8(xq, t))
    x = long_f32(5, 2, 256, 64, t)
    np.testing.assert_array_equal(eo.mha_long(cu(x)).cpu().numpy(), oracle.mha(x, t))
    eo.close()
