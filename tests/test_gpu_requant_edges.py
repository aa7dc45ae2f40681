"""Every form of the requantisation step on the GPU, at the accumulators where forms differ and at the edges of the
range the stream kernels accept: bit equality with the numpy definition (mha_heads_ref, held to the C oracle by
tests/test_requant_cpu.py) on crafted blobs (requant_common), through every route that accepts the blob.

Forms and the routes that reach them: the block kernels ita_mha_kernel<E, H> / ita_ffn_kernel
(mha with taps, ffn, and everything on a blob without stream images) requantise in plain C++; the stream kernel
(mha without taps, mha_q8, encoder_layer) and the long kernels (mha_long_q8, mha_long) run the two-rounding or the
single-rounding asm form as ita_load_weights' proof decides, the ReLU form at fc1 and the block-output form at fc2.
Each test asserts through Engine.layer_forms that the form it names is the one that ran.  test_requant_cpu.py asserts
that the accumulators the cases are about occur, so a run here cannot pass by missing them."""
import numpy as np
import pytest

import requant_common as rc
from conftest import golden_files
from drone_oa_iree_vit_accelerator_amd import host, params
from gpu_support import UNSUPPORTED, cu, refused_untouched

pytestmark = pytest.mark.gpu

MHA_TAPS, FFN_TAPS = rc.MHA_TAPS, ("x_q", "h", "out_q")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _routes(eng, c, stream):
    """every route that accepts the case's blob against the definition -> the names of the routes that differ.
    stream: the blob has its stream images, so the tap-less routes run on the stream kernels and the int8 entries
    accept it; else everything runs on the block kernels and the int8 entries must refuse."""
    exp = c.expect()
    x = cu(c.x)
    bad = []

    def same(name, got, want):
        if not np.array_equal(got.cpu().numpy(), want, equal_nan=True):
            bad.append(name)

    out, taps, _ = exp["mha"]
    gy, gt = eng.mha(x, taps=True)
    for k in MHA_TAPS:
        same(f"mha taps:{k}", gt[k], taps[k])
    same("mha taps", gy, out)
    same("mha", eng.mha(x), out)
    fout, ftaps, _ = exp["ffn"]
    fy, ft = eng.ffn(x, taps=True)
    for k in FFN_TAPS:
        same(f"ffn taps:{k}", ft[k], ftaps[k])
    same("ffn taps", fy, fout)
    same("ffn", eng.ffn(x), fout)
    same("encoder_layer", eng.encoder_layer(x), exp["x2"])
    lout, ltaps, _ = exp["long"]
    xq, xlq = cu(taps["x_q"]), cu(ltaps["x_q"])
    if stream:
        same("mha_q8", eng.mha_q8(xq), taps["out_q"])
        same("mha_long_q8", eng.mha_long_q8(xlq), ltaps["out_q"])
        same("mha_long", eng.mha_long(cu(exp["x_long"])), lout)
    else:
        if not refused_untouched(eng, host.lib().ita_mha_q8, xq):
            bad.append("mha_q8 refusal")
        if not refused_untouched(eng, host.lib().ita_mha_long_q8, xlq, 256):
            bad.append("mha_long_q8 refusal")
        with pytest.raises(host.ITAError, match=UNSUPPORTED):
            eng.mha_long(cu(exp["x_long"]))
    return bad


@pytest.mark.parametrize("E,site,j", rc.rounding_ids(), ids=lambda v: str(v))
def test_rounding(torch_cuda, E, site, j):
    """a. the accumulators on which one and two roundings differ, their neighbours, and the neighbours of the ties at
    both ends of the clamp and at zero, at one site; two refused multipliers (the two-rounding instantiation runs), two
    admitted ones and a power of two, where every wanted accumulator is a true tie (the single-rounding one runs)"""
    c = rc.rounding_case(E, site, j)
    exp = c.expect()
    eng = host.Engine(c.blob(), device=0)
    forms = eng.layer_forms()
    assert forms["fast_sites"] == rc.expected_mask(c), (forms, c.name)
    assert forms["fast"] == (c.kind != "refused" or site in rc.FFN_SITES)
    assert forms["attn_image"] and forms["layer_image"] and not forms["tok_image"]
    n = c.present(rc.site_accumulators(c, exp))
    print(f"{c.name}: m = {float(c.m)!r}, {'single' if forms['fast'] else 'two'}-rounding stream kernels, "
          f"{n} of {len(c.want)} wanted accumulators present, {len(c.diff)} of them differing")
    assert n == len(c.want)
    bad = _routes(eng, c, stream=True)
    eng.close()
    assert not bad, f"{c.name}: differs from the definition on {bad}"
    assert len(np.unique(exp["mha"][0].reshape(-1, E), axis=0)) > 64      # the crafted rows are not the only content


@pytest.mark.parametrize("E,site", [(64, "L"), (64, "O"), (128, "Q")], ids=lambda v: str(v))
def test_rounding_two_heads(torch_cuda, E, site):
    """a refused multiplier's accumulators through ita_mha_kernel<E, 2>: a multi-head blob has no stream images"""
    c = rc.rounding_case(E, site, 0, H=2)
    exp = c.expect()
    eng = host.Engine(c.blob(), device=0)
    assert eng.H == 2
    forms = eng.layer_forms()
    assert forms == dict(fast_sites=0, fast=False, attn_image=False, layer_image=False, tok_image=False)
    acc = exp["mha"][2][site]
    n = c.present(acc[:, 0] if site == "L" else acc)
    print(f"{c.name} H = 2: {n} of {len(c.want)} wanted accumulators present")
    assert n == len(c.want) and c.diff
    bad = _routes(eng, c, stream=False)
    eng.close()
    assert not bad, f"{c.name} H = 2: differs from the definition on {bad}"


@pytest.mark.parametrize("E,site,kind", rc.range_ids(), ids=lambda v: str(v))
def test_range(torch_cuda, E, site, kind):
    """b. one weight row pair at 2^22 - 1 / 2^22, or at a product just under / at 32000, with inputs that drive the
    accumulator to the extreme of both signs: inside, the stream images exist and every stream route equals the
    definition (saturated values are +127 / -128, never wrapped); outside, they do not exist, the block kernels compute
    the same, and the int8 entries refuse before any launch"""
    c = rc.range_case(E, site, kind)
    exp = c.expect()
    eng = host.Engine(c.blob(), device=0)
    forms = eng.layer_forms()
    inside = rc.range_inside(c)
    acc = rc.site_accumulators(c, exp)
    print(f"{c.name}: m = {float(c.m)!r}, accumulators in [{acc.min()}, {acc.max()}], forms {forms}")
    assert c.present(acc) == 2
    ffn_site = site in rc.FFN_SITES      # an FFN row out of range costs the whole-layer image only
    if ffn_site:                         # the stream kernel's fc1 / fc2 forms run in encoder_layer alone: the edge is reached there too
        assert c.present(exp["ffn_x1"][2][site]) == 2
    assert forms["attn_image"] == (inside or ffn_site) and forms["layer_image"] == inside, forms
    if not forms["attn_image"]:
        assert forms["fast_sites"] == 0
    bad = _routes(eng, c, stream=forms["attn_image"])
    eng.close()
    assert not bad, f"{c.name}: differs from the definition on {bad}"


STREAM_FIXTURES = [(64, "blocks_E64_seed2_B1.npz", False), (64, "vitlstm_E64_seed0_B2.npz", True),
                   (128, "blocks_E128_seed0_B1.npz", False), (128, "vit2l_us_E128_s1_B2.npz", True)]


@pytest.mark.parametrize("E,name,fast", STREAM_FIXTURES, ids=lambda v: str(v))
def test_stream_kernel_inputs(torch_cuda, oracle, E, name, fast):
    """c. the input of test_blocks_random_batch_and_saturation (zeros, saturating rows, a 1e30 row, exact ties 0.5 s and
    1.5 s; 37 frames) through the tap-less routes, which run the stream kernel: on a fixture whose six multipliers are
    all admitted and on one with a refused site"""
    d = params.load_fixture(golden_files(name)[0])
    t = {**params.attention_tensors(d, "attn0.", 0), **params.ffn_tensors(d, "ffn0.", 0)}
    t.update({k: v for k, v in rc.base(E)[0].items() if k.startswith("norm")})
    eng = host.Engine(params.pack_blob(t, E=E, has_tail=False), device=0)
    forms = eng.layer_forms()
    assert forms["fast"] == fast and forms["attn_image"] and forms["layer_image"], forms
    rs = np.random.RandomState(5)
    B = 37
    x = rs.standard_normal((B, 128, E)).astype(np.float32)
    s = np.float32(float(d["attn0.quant.scale"]))
    x[0], x[1], x[2] = 0.0, 50.0, -50.0
    x[3, :, ::2] *= 30.0
    x[4, 5] = 1e30
    x[5], x[6] = np.float32(0.5) * s, np.float32(1.5) * s
    oy, otaps = oracle.mha(x, t, taps=True)
    assert (otaps["x_q"][5] == 0).all() and (otaps["x_q"][6] == 2).all() and (otaps["x_q"][4, 5] == 127).all()   # ties to even
    xc = cu(x)
    np.testing.assert_array_equal(eng.mha(xc).cpu().numpy(), oy)
    np.testing.assert_array_equal(eng.mha_q8(cu(otaps["x_q"])).cpu().numpy(), otaps["out_q"])
    np.testing.assert_array_equal(eng.ffn(xc).cpu().numpy(), oracle.ffn(x, t))
    x1 = oracle.add_ln(x, oy, t["norm1_0.w"], t["norm1_0.b"])
    x2 = oracle.add_ln(x1, oracle.ffn(x1, t), t["norm2_0.w"], t["norm2_0.b"])
    got = eng.encoder_layer(xc).cpu().numpy()
    print(f"{name}: the 1e30 token's row: oracle {x2[4, 5, :4]}, engine {got[4, 5, :4]}")
    np.testing.assert_array_equal(got, x2)
    eng.close()
