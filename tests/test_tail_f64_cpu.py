"""The references of tests/tail_f64_common.py, checked on the CPU: truth64 against the reference's own fixtures, the fold
G0 against the unfolded float64 graph, the split model against ita_weights_load.h's rules, every case against the regime
it is named for, and -- the sensitivity argument of test_gpu_tail_f64.py -- every mutant of split64 against the bound the
GPU result is held to: a kernel that dropped a cross term, flushed f16 subnormals, skipped a k-step or evaluated tanh as a
ratio would land outside 2 x bound on the cases listed in SENSITIVITY."""
import numpy as np
import pytest

import tail_f64_common as tc
from conftest import golden_files
from drone_oa_iree_vit_accelerator_amd import params, synth

FIX_VIT = golden_files("vitlstm_*.npz")
SENSITIVITY = {
    "no_x_lo": ("A0", "A1", "W1", "W4_i", "W4_f", "W4_g", "W4_o"),
    "no_w_lo": ("A0", "A1", "W1", "W4_i", "W4_f", "W4_g", "W4_o"),
    "flush_f16_subnormals": ("A1", "W1"),
}


def _subnormal(a):
    a = np.abs(np.asarray(a, np.float64))
    return (a > 0) & (a < tc.F16_MIN_NORMAL)


def _frac_subnormal(a):
    a = np.asarray(a, np.float64)
    return float(_subnormal(a).sum()) / max(int((a != 0).sum()), 1)


# ------------------------------------------------------------------ truth64 and the fold
@pytest.mark.parametrize("path", FIX_VIT, ids=[p.split("/")[-1][:-4] for p in FIX_VIT])
def test_truth64_meets_fixture(path):
    """from the reference's own x2: its conv map and decoder output within 2e-5 (test_float_stages), its velocity within
    1e-5 and its state within 5e-4 (test_forward_from_reference_tokens)"""
    d = params.load_fixture(path)
    fp = synth.float_params(int(d["meta.seed"]), E=64)
    B = d["s0.x2"].shape[0]
    z = np.zeros((3, B, 128), np.float32)
    np.testing.assert_allclose(tc.feat64(d["s0.x2"], fp).reshape(-1, 9, 16, 32), d["s0.tail.conv"], atol=2e-5, rtol=0)
    dec = tc.front_truth(fp, d["s0.x2"])
    np.testing.assert_allclose(dec, d["s0.dec"], atol=2e-5, rtol=0)
    t = tc.head_truth(fp, dec, d["in0.desvel"], d["in0.quat"], z, z)
    for key, got, tol in (("s0.vel", t["vel"], 1e-5), ("s0.h", t["h"], 5e-4), ("s0.c", t["c"], 5e-4)):
        print(f"{key}: max |truth64 - fixture| = {np.abs(got - d[key]).max():.3e}")
        np.testing.assert_allclose(got, d[key], atol=tol, rtol=0, err_msg=key)


def test_fold_equals_unfolded_graph():
    """G0 . x2 + bias'' (built by the transposed maps) against W_ih0[:, :512] . dec64(x2) (the forward statement), float64"""
    fp = tc.seed0_params()
    x2 = tc.case("A0")["x2"][:2]
    wf, bias = tc.wfold64(fp)
    dec = tc.front_truth(fp, x2)
    got = x2.reshape(2, -1).astype(np.float64) @ wf.T + bias
    np.testing.assert_allclose(got, dec, atol=1e-12 * np.abs(dec).max(), rtol=0)
    g0, _, b0 = tc.g0_split(fp)
    assert g0.dtype == np.float32 and g0.shape == (512, 8192)
    w0 = fp["lstm.weight_ih_l0"][:, :512].astype(np.float64)
    np.testing.assert_allclose(x2.reshape(2, -1).astype(np.float64) @ g0.astype(np.float64).T + b0, dec @ w0.T, atol=2e-6, rtol=0)


# ------------------------------------------------------------------ the split model
def _weight_tensors(fp):
    yield "G0", tc.g0_split(fp)[0]
    yield "rem0", tc.rem0_weights(fp)
    for l in (1, 2):
        yield f"cat{l}", tc.cat_weights(fp, l)


@pytest.mark.parametrize("name", ["A0", "W1", "W2"])
def test_split_scale_and_halves(name):
    """split_scale_exp: e = 10 - frexp(max|w|).exp, so max|w| 2^e lies in [512, 1024); hi + lo gives the scaled operand back
    to max(2^-22 |v|, 2^-25)"""
    fp = tc.case(name)["fp"]
    for what, w in _weight_tensors(fp):
        hi, lo, e = tc.split_weights(w)
        mx = float(np.abs(w).max())
        assert e == 10 - int(np.frexp(mx)[1]), what
        assert 512.0 <= mx * 2.0 ** e < 1024.0, what
        v = w.astype(np.float64) * 2.0 ** e
        err = np.abs(hi.astype(np.float64) + lo.astype(np.float64) - v)
        assert np.isfinite(hi.astype(np.float64)).all(), what
        assert (err <= np.maximum(2.0 ** -22 * np.abs(v), 2.0 ** -25)).all(), (what, float(err.max()))


def test_split_of_activations():
    """split_f16 unscaled, over the cases' activation ranges (f16 subnormal halves included): hi + lo to max(2^-22 |v|, 2^-25)"""
    for name in ("A0", "A1", "A2", "A3"):
        v = tc.case(name)["x2"].astype(np.float64)
        hi, lo = tc.split_f16(v)
        err = np.abs(hi.astype(np.float64) + lo.astype(np.float64) - v)
        assert (err <= np.maximum(2.0 ** -22 * np.abs(v), 2.0 ** -25)).all(), name


def test_split_scale_exp_edges():
    assert tc.split_scale_exp(0.0) == 0
    for mx, e in ((1.0, 9), (0.999, 10), (512.0, 0), (1023.9, 0), (1024.0, -1), (2.0 ** -20, 29)):
        assert tc.split_scale_exp(mx) == e, mx


# ------------------------------------------------------------------ every case is in the regime it is named for
def test_regime_a1_lo_halves_subnormal():
    cs = tc.case("A1")
    for what, a in (("x2", cs["x2"]), ("h_in", cs["h_in"]), ("quat", cs["quat"])):
        hi, lo = tc.split_f16(a)
        assert _frac_subnormal(lo) > 0.9, what
        assert _frac_subnormal(hi) < 0.1, what


def test_regime_a2_hi_halves_straddle_f16_min_normal():
    hi, lo = tc.split_f16(tc.case("A2")["x2"])
    f = _frac_subnormal(hi)
    assert 0.1 < f < 0.9, f
    assert _frac_subnormal(lo) == 1.0   # what is left of the lo halves is all subnormal


def test_regime_a3_large_activations_normal_lo():
    cs = tc.case("A3")
    hi, lo = tc.split_f16(cs["x2"])
    assert _frac_subnormal(lo) < 0.1 and np.isfinite(hi.astype(np.float64)).all()
    top = 16.0 * tc.ln_ceiling(cs["fp"])
    assert 55.0 < np.abs(tc.x2_fixture(8) * 16.0).max() < 65.0
    assert int((np.abs(cs["x2"]) == np.float32(top)).sum()) == 4 and top < 65504.0


def test_regime_a4_impulses_read_columns_of_g0():
    cs = tc.case("A4")
    x = cs["x2"].reshape(len(tc.IMPULSE_K), -1)
    assert (np.count_nonzero(x, axis=1) == 1).all() and not cs["h_in"].any() and not cs["c_in"].any()
    fp = cs["fp"]
    wf, bias = tc.wfold64(fp)
    g0 = fp["lstm.weight_ih_l0"][:, :512].astype(np.float64) @ wf
    pre0 = tc.refs("A4")[0]["pre"][0]
    rest = tc.head_truth(fp, np.tile(bias, (len(x), 1)), cs["desvel"], cs["quat"], cs["h_in"], cs["c_in"], upto=1)["pre"][0]
    for b, k in enumerate(tc.IMPULSE_K):
        assert x[b, k] == np.float32(1.0 + 2.0 ** -12)
        np.testing.assert_allclose(pre0[b] - rest[b], g0[:, k] * (1.0 + 2.0 ** -12), atol=1e-13, rtol=0)


def test_regime_w1_dominant_rows_set_the_scale():
    cs = tc.case("W1")
    fp, base = cs["fp"], tc.seed0_params()
    for (what, w), (_, w0), l in zip(_weight_tensors(fp), _weight_tensors(base), (0, 0, 1, 2)):
        row = tc.W1_ROWS[l]
        hi, lo, e = tc.split_weights(w)
        assert e <= tc.split_weights(w0)[2] - 8, what   # the scaled row sets the exponent
        assert int(np.abs(w).max(axis=1).argmax()) == row, what
        others = np.delete(lo, row, axis=0)
        f = _frac_subnormal(others)
        print(f"W1 {what}: e = {e}, {100 * f:.1f} % of the other rows' non-zero lo halves are f16-subnormal")
        assert f > 0.5, (what, f)
    assert all(not cs["mask"][l, tc.W1_ROWS[l] % 128] and cs["mask"][l].sum() == 127 for l in range(3))


def test_regime_w2_small_lstm_weights_large_decoder():
    fp, base = tc.case("W2")["fp"], tc.seed0_params()
    for l in range(3):
        for nm in ("weight_ih", "weight_hh"):
            np.testing.assert_array_equal(fp[f"lstm.{nm}_l{l}"] * np.float32(256.0), base[f"lstm.{nm}_l{l}"])
    np.testing.assert_array_equal(fp["decoder.weight"], base["decoder.weight"] * np.float32(64.0))


def test_regime_w3_saturation_reached():
    """every gate of every layer sees every target on frame 0 (exactly there: the bias is solved for it), the other frames
    differ by c_in alone; the exp2 argument leaves +-128 on both sides; the ratio form of tanh goes non-finite"""
    cs = tc.case("W3")
    t = tc.refs("W3")[0]
    tgt = np.array(tc.SAT_TARGETS)
    for l in range(3):
        pre = t["pre"][l][0].reshape(4, 128)
        for g in range(4):
            near = np.abs(pre[g][:, None] - tgt[None, :]).argmin(axis=1)
            assert set(near) == set(range(13)), (l, g)
            assert (np.abs(pre[g] - tgt[near]) <= 1e-7 + 2.0 ** -23 * np.abs(tgt[near])).all(), (l, g)
        assert (np.abs(t["pre"][l]) * 1.4426950408889634 > 128.0).any()
        assert (np.abs(t["pre"][l][:, 256:384]) > 44.5).any()
    assert set(np.unique(cs["c_in"])) == {0.0, 1.0, -1.0, 20.0, -20.0, 50.0, -50.0} and np.signbit(cs["c_in"][:, 1]).all()
    h = cs["h_in"]
    assert (h == 1).any() and (h == -1).any() and ((h == 0) & np.signbit(h)).any() and ((h != 0) & (np.abs(h) < 1e-2)).any()
    for res in (t, tc.refs("W3")[1], tc.refs("W3")[2]):
        assert all(np.isfinite(v).all() for v in tc.tensors(res).values())
    bad = tc.split64(cs, "tanh_ratio")
    assert not np.isfinite(bad["c"]).all() and not np.isfinite(bad["vel"]).all()


@pytest.mark.parametrize("name", ["W4_i", "W4_f", "W4_g", "W4_o"])
def test_regime_w4_g_preactivation_reaches_the_output(name):
    """i = o = 1 and c_in = 0: c[l] = tanh(g_l), h[l] = tanh(c[l]); the g slot holds the named gate's rows of the seed-0 weights"""
    cs = tc.case(name)
    t = tc.refs(name)[0]
    for l in range(3):
        g = t["pre"][l][:, 256:384]
        np.testing.assert_allclose(t["c"][l], np.tanh(g), atol=1e-12, rtol=0)
        np.testing.assert_allclose(t["h"][l], np.tanh(np.tanh(g)), atol=1e-12, rtol=0)
        src = "ifgo".index(name[-1]) * 128
        for nm in ("weight_ih", "weight_hh"):
            np.testing.assert_array_equal(cs["fp"][f"lstm.{nm}_l{l}"][256:384], tc.seed0_params()[f"lstm.{nm}_l{l}"][src:src + 128])


# ------------------------------------------------------------------ sensitivity: what the bound would catch
def _ratios(name, mutant):
    cs = tc.case(name)
    t, _, _, b, _, _ = tc.refs(name)
    em = tc.errors(tc.split64(cs, mutant), t, cs["mask"])
    return {n: em[n] / b[n] for n in tc.TENSORS}


@pytest.mark.parametrize("mutant,name", [(m, n) for m, ns in SENSITIVITY.items() for n in ns])
def test_sensitivity(mutant, name):
    r = _ratios(name, mutant)
    print(f"{name} {mutant}: error / bound = " + ", ".join(f"{n} {v:.1f}" for n, v in r.items()))
    assert max(r.values()) > 2.0


@pytest.mark.parametrize("k0", [0, 32, 64, 992, 1024, 8160])
def test_sensitivity_skipped_k_step(k0):
    """A4: each impulse sits in one k-step of 32; the model that leaves that step out loses the column"""
    r = _ratios("A4", ("skip_k_step", k0))
    assert max(r.values()) > 2.0
    hit = [b for b, k in enumerate(tc.IMPULSE_K) if k0 <= k < k0 + 32]
    cs, t = tc.case("A4"), tc.refs("A4")[0]
    d = np.abs(tc.split64(cs, ("skip_k_step", k0))["c"][0] - t["c"][0]).max(axis=1)
    assert hit and all((d[b] > 2.0 * tc.refs("A4")[3]["c0"]) == (b in hit) for b in range(len(tc.IMPULSE_K))), (k0, hit)


def test_split_design_within_its_own_bound():
    """the unmutated model (and the f32 oracle) sit inside every bound by construction: at most a third of it"""
    for name in tc.CASES:
        cs = tc.case(name)
        t, o, s, b, _, _ = tc.refs(name)
        for res in (o, s):
            e = tc.errors(res, t, cs["mask"])
            assert all(e[n] <= b[n] / 3.0 for n in tc.TENSORS), name


# ------------------------------------------------------------------ R1
def test_recurrence_references():
    """64 steps with the forget gate held open (mean f above 0.9: the state is remembered, and so is every earlier step's
    rounding): every step has finite references, and both references stay within a third of the step's bound"""
    cs, steps = tc.recurrence()
    assert len(steps) == tc.R1_STEPS
    f = 1.0 / (1.0 + np.exp(-steps[0][0]["pre"][:, :, 128:256]))
    assert f.mean() > 0.9
    for t, (truth, b, e32, esp) in enumerate(steps):
        assert all(np.isfinite(v).all() for v in tc.tensors(truth).values()), t
        assert all(np.isfinite(b[n]) and 3.0 * max(e32[n], esp[n]) <= b[n] for n in tc.TENSORS), (t, b)
    print("R1 bound on c2 at steps 0, 15, 63:", [f"{steps[t][1]['c2']:.2e}" for t in (0, 15, 63)])
