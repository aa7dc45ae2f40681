"""The fused requantisation form on the GPU (ita_stream_kernel<..., FUSED>): bit equality with the definition on layers
that run it -- under accumulator bases that are NOT 0x4B400000 -- and on layers that do not, with the diagnostic
switch ITA_FUSED_SITES=0 in a fresh process, at one and three frames (both column-sum parities, the last-frame path).

Crafted blobs: requant_common's rounding cases put the neighbours of every rounding tie of a site into its accumulators
by a zero weight row and the wanted value as the bias, so under the fused form the accumulator is C_site + that value;
the travel_in range cases drive a row to the +-2^15 edge of the 16-bit travel format.  Which of them run fused is
decided here on the CPU the way the loader decides it (requant_fused_common.proven) and asserted on the engine.
Flavours: E = 64 with the tokenizer in front (forward), the E = 64 and E = 128 layers (encoder_layer), ita_mha_int8
and ita_mha_q8."""
import os
import subprocess
import sys

import numpy as np
import pytest

import requant_common as rc
from conftest import REPO, golden_files
from drone_oa_iree_vit_accelerator_amd import host, params, synth
from gpu_support import cu
from requant_fused_common import differs, k_of, proven

pytestmark = pytest.mark.gpu

CRAFTED = [("round", E, s, j) for E in (64, 128) for s in host.FUSED_SITES for j in (2, 4)] + \
          [("range", E, s, "travel_in") for E in (64, 128) for s in ("Q", "K", "V", "L")]
FIXTURES = ["vitlstm_E64_seed0_B2.npz", "blocks_E64_seed2_B1.npz", "blocks_E128_seed0_B1.npz", "vit2l_us_E128_s1_B2.npz"]


@pytest.fixture(scope="module", autouse=True)
def torch_cuda():
    """torch's HIP runtime is up before the library makes its first HIP call, as in every GPU test here"""
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _case(kind, E, site, j):
    return rc.rounding_case(E, site, j) if kind == "round" else rc.range_case(E, site, j)


def _expected_sites(t):
    """the loader's decision per fused site of a blob whose rows leave the base its full room: {site: C or None}"""
    return {s: proven(rc.multiplier_of(t, s), logits=(s == "L")) for s in host.FUSED_SITES}


def _expect_fused(t):
    sites = _expected_sites(t)
    fast = all(host.fast_site_ok(rc.multiplier_of(t, s)) for s in rc.ATTN_SITES)
    return sites, fast and all(C is not None for C in sites.values())


def _check_forms(eng, t, off=False):
    """the engine's fused mask, bases and constants against the CPU's decision and the exact re-computation"""
    sites, want = _expect_fused(t)
    lf = eng.layer_fused()
    if off:
        assert lf["fused_sites"] == 0 and not lf["fused"], lf
        return False
    assert lf["fused"] == want, (lf, sites)
    for i, s in enumerate(host.FUSED_SITES):
        assert bool(lf["fused_sites"] >> i & 1) == (sites[s] is not None), (s, lf, sites)
        if sites[s] is not None:
            m, lg = rc.multiplier_of(t, s), s == "L"
            assert lf["C"][i] == sites[s] and lf["K"][i] == k_of(m, sites[s], 12615680 if lg else 12583040), (s, lf)
            assert differs(m, lf["C"][i], lf["K"][i], lg).size == 0, s
    # fc1's fused ReLU form: its own proof, on top of a fused layer with a whole-layer image
    m1 = rc.multiplier_of(t, "fc1")
    c1 = proven(m1, relu=True)
    assert lf["fused_relu"] == (want and c1 is not None and eng.layer_forms()["layer_image"]), (lf, c1)
    if lf["fused_relu"]:
        assert lf["C"][5] == c1 and lf["K"][5] == k_of(m1, c1, 12582912) and differs(m1, c1, lf["K"][5], relu=True).size == 0
    else:
        assert lf["C"][5] == host.ACC_BIAS
    return want


def test_case_selection():
    """enough of the crafted cases run fused, under bases away from the default, and some do not"""
    fused = [(c, _expect_fused(_case(*c).t)) for c in CRAFTED]
    n_fused = sum(f for _, (_, f) in fused)
    moved = sum(f and sites[c[2]] != host.ACC_BIAS for c, (sites, f) in fused)
    print(f"{len(CRAFTED)} crafted cases: {n_fused} fused, {moved} of them with the case's own site off the default base")
    assert n_fused >= 8 and moved >= 6 and n_fused < len(CRAFTED)
    assert any(f and c[0] == "range" for c, (_, f) in fused)
    fx = [_expect_fused(_fixture_tensors(n)[1])[1] for n in FIXTURES]
    assert fx[0] and not fx[1], fx          # the bench blob's layer is fused; blocks_E64_seed2 has refused sites


@pytest.mark.parametrize("kind,E,site,j", CRAFTED, ids=lambda v: str(v))
def test_crafted(kind, E, site, j):
    c = _case(kind, E, site, j)
    exp = c.expect()
    acc = rc.site_accumulators(c, exp)
    assert c.present(acc) == (len(c.want) if kind == "round" else 2)
    eng = host.Engine(c.blob(), device=0)
    fused = _check_forms(eng, c.t)
    forms = eng.layer_forms()
    assert forms["attn_image"] and forms["layer_image"]
    print(f"{c.name}: m = {float(c.m)!r}, fused {fused}, bases {[C - host.ACC_BIAS for C in eng.layer_fused()['C']]}")
    x = cu(c.x)
    out, taps, _ = exp["mha"]
    np.testing.assert_array_equal(eng.mha(x).cpu().numpy(), out)
    np.testing.assert_array_equal(eng.mha_q8(cu(taps["x_q"])).cpu().numpy(), taps["out_q"])
    np.testing.assert_array_equal(eng.encoder_layer(x).cpu().numpy(), exp["x2"])
    # the long kernels read the same layer's default-base image
    np.testing.assert_array_equal(eng.mha_long_q8(cu(exp["long"][1]["x_q"])).cpu().numpy(), exp["long"][1]["out_q"])
    eng.close()


def _fixture_tensors(name):
    d = params.load_fixture(golden_files(name)[0])
    E = 128 if "E128" in name else 64
    t = {**params.attention_tensors(d, "attn0.", 0), **params.ffn_tensors(d, "ffn0.", 0)}
    t.update({k: v for k, v in rc.base(E)[0].items() if k.startswith("norm")})
    return E, t, d


def run_flavours(off=False):
    """every stream-kernel flavour at B = 1 and B = 3 against the C oracle, bit for bit; off: ITA_FUSED_SITES=0 is set,
    no layer may run fused.  Returns {fixture: fused}."""
    import torch
    from oracle import oracle
    oracle.build()
    ran = {}
    rs = np.random.RandomState(9)
    for name in FIXTURES:
        E, t, d = _fixture_tensors(name)
        eng = host.Engine(params.pack_blob(t, E=E, has_tail=False), device=0)
        ran[name] = _check_forms(eng, t, off)
        for B in (1, 3):
            x = (rs.standard_normal((B, 128, E)) * 1.5).astype(np.float32)
            x[B - 1, ::3] *= 20.0                                   # saturating rows in the last frame
            oy, otaps = oracle.mha(x, t, taps=True)
            np.testing.assert_array_equal(eng.mha(cu(x)).cpu().numpy(), oy, err_msg=f"{name} mha B={B}")
            np.testing.assert_array_equal(eng.mha_q8(cu(otaps["x_q"])).cpu().numpy(), otaps["out_q"], err_msg=f"{name} q8 B={B}")
            x1 = oracle.add_ln(x, oy, t["norm1_0.w"], t["norm1_0.b"])
            x2 = oracle.add_ln(x1, oracle.ffn(x1, t), t["norm2_0.w"], t["norm2_0.b"])
            np.testing.assert_array_equal(eng.encoder_layer(cu(x)).cpu().numpy(), x2, err_msg=f"{name} layer B={B}")
        eng.close()
    # E = 64 with the tokenizer in front: the whole model's blob, x2 of forward against the oracle on the kernel's own tokens
    fx = params.load_fixture(golden_files("vitlstm_E64_seed0_B2.npz")[0])
    fp = synth.float_params(0, E=64)
    eng = host.Engine(params.blob_from_record(fx, fp, E=64), device=0)
    lf = eng.layer_fused()
    assert lf["fused"] == (not off) and lf["fused_relu"] == (not off) and eng.layer_forms()["tok_image"], lf
    t = {**params.attention_tensors(fx, "attn0.", 0), **params.ffn_tensors(fx, "ffn0.", 0)}
    fr = synth.frames(4, 3)
    for B in (1, 3):
        _, _, ta = eng.forward(torch.from_numpy(fr["img_u8"][:B]).cuda(), torch.from_numpy(fr["desvel"][:B]).cuda(),
                               torch.from_numpy(fr["quat"][:B]).cuda(), taps=True)
        tok = ta["tokens"].cpu().numpy()
        x1 = oracle.add_ln(tok, oracle.mha(tok, t), fp["norms1.0.weight"], fp["norms1.0.bias"])
        x2 = oracle.add_ln(x1, oracle.ffn(x1, t), fp["norms2.0.weight"], fp["norms2.0.bias"])
        np.testing.assert_array_equal(ta["x2"].cpu().numpy(), x2, err_msg=f"tokenizer flavour B={B}")
    eng.close()
    ran["vitlstm blob"] = lf["fused"]
    return ran


def test_flavours_fused():
    ran = run_flavours()
    print(ran)
    assert ran["vitlstm_E64_seed0_B2.npz"] and ran["vitlstm blob"] and not ran["blocks_E64_seed2_B1.npz"]
    assert any(ran[n] for n in FIXTURES if "E128" in n), ran       # an E = 128 layer runs fused too


def test_flavours_with_the_switch_off():
    """ITA_FUSED_SITES=0 in a fresh process: the mask is ANDed onto the proven sites, every layer keeps its fast or exact
    form, same results"""
    env = dict(os.environ, ITA_FUSED_SITES="0", PYTHONPATH=os.pathsep.join([os.path.join(REPO, "tests"), REPO]))
    code = "import torch; assert torch.cuda.is_available(); import test_gpu_requant_fused as t; r = t.run_flavours(off=True); assert not any(r.values()), r; print('off ok', r)"
    r = subprocess.run([sys.executable, "-c", code], cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "off ok" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


def test_switch_cannot_turn_a_site_on():
    """ITA_FUSED_SITES=31 on a layer with refused sites: still not fused (mask &= proven)"""
    env = dict(os.environ, ITA_FUSED_SITES="31", PYTHONPATH=os.pathsep.join([os.path.join(REPO, "tests"), REPO]))
    code = ("import torch; assert torch.cuda.is_available()\n"
            "import test_gpu_requant_fused as t\n"
            "from drone_oa_iree_vit_accelerator_amd import host, params\n"
            "E, tt, d = t._fixture_tensors('blocks_E64_seed2_B1.npz')\n"
            "eng = host.Engine(params.pack_blob(tt, E=E, has_tail=False), device=0)\n"
            "t._check_forms(eng, tt); lf = eng.layer_fused(); assert not lf['fused'] and lf['fused_sites'] != 31, lf\n"
            "eng.close(); print('and ok')\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "and ok" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
