"""ita_fusion_tail_large over every kernel it dispatches to (GPU, -m gpu; the shapes and what selects them: tail_common.py).

  matrix      each case against the C oracle (f32 fmaf chain) AND the float64 definition (tail_common.tail_f64), both
              within the tolerance of test_tail_large.py, 2e-5 max|want|;
  batch       ita_tail_big_kernel at B = 3: two runs bit-identical, frame b = the same frame run alone, bit for bit;
  exact       integer data on the pixel-shuffle channels (result == float64, zero tolerance: an index error cannot hide
              inside 2e-5) and power-of-two weight scaling (loading w 2^k gives exactly 2^k times the output);
  magnitude   tokens N(0,1) 2^p: the tolerance holds for p = -6, 0, +12; p = -10, -12 finite (figures: DESIGN.md);
  life cycle  the loader's and the call's refusals return their ITA_ERR_* code and leave the handle usable; a reload
              to another (E, CO) gives a fresh engine's bits.
The tests print their figures (pytest -s) before they assert."""
import ctypes as C

import numpy as np
import pytest

import tail_common as tc
from drone_oa_iree_vit_accelerator_amd import host

pytestmark = pytest.mark.gpu

ITA_ERR_INVALID_ARG, ITA_ERR_NO_WEIGHTS, ITA_ERR_UNSUPPORTED = -1, -3, -4    # include/ita_mi355x.h: ita_status


def _run(c, th, tw):
    import torch
    eng = host.FusionTailLarge(c["conv_w"], c["conv_b"], device=0)
    out = eng(torch.from_numpy(c["x"]).cuda(), th, tw)
    torch.cuda.synchronize()
    res = out.cpu().numpy()
    eng.close()
    return res


def _report(tag, shape, got, want, want64):
    """prints and returns the two errors relative to max|want| (the unit of the tolerance)"""
    e32 = float(np.abs(got - want).max() / np.abs(want).max())
    e64 = float(np.abs(got.astype(np.float64) - want64).max() / np.abs(want64).max())
    print(f"\nTAILERR {tag} {tc.variant(*shape)} {tc.case_id(shape)} vs_oracle {e32:.3e} vs_f64 {e64:.3e}")
    return e32, e64


# ------------------------------------------------------------------------------------------ matrix
@pytest.mark.parametrize("shape", tc.MATRIX, ids=[f"{tc.case_id(s)}-{tc.variant(*s)}" for s in tc.MATRIX])
def test_gpu_tail_matrix_vs_oracle_and_f64(oracle, shape):
    E, th, tw, co = shape
    B = 1 if th * tw > 512 else 2
    c = tc.case(shape, B)
    want = oracle.tail_general(c["x"], th, tw, c["conv_w"], c["conv_b"])
    want64 = tc.want_f64(shape, B)
    got = _run(c, th, tw)
    assert got.shape == want.shape
    e32, e64 = _report("matrix", shape, got, want, want64)
    assert np.isfinite(got).all()
    assert e32 <= 2e-5      # f16x3 MFMA vs the f32 fmaf chain (test_tail_large.py's tolerance)
    assert e64 <= 2e-5      # and vs the float64 definition


# ------------------------------------------------------------------------------------------ batch independence
@pytest.mark.parametrize("shape", tc.BIG, ids=[f"{tc.case_id(s)}-{tc.variant(*s)}" for s in tc.BIG])
def test_gpu_tail_big_batch_independent(shape):
    import torch
    E, th, tw, co = shape
    c = tc.case(shape, 3, seed=22)
    eng = host.FusionTailLarge(c["conv_w"], c["conv_b"], device=0)
    x = torch.from_numpy(c["x"]).cuda()
    full = eng(x, th, tw)
    again = eng(x, th, tw)
    assert torch.equal(full, again)
    for b in range(3):
        alone = eng(x[b:b + 1].contiguous(), th, tw)
        assert torch.equal(full[b], alone[0]), f"frame {b}"
    eng.close()


# ------------------------------------------------------------------------------------------ exact
@pytest.mark.parametrize("shape", tc.EXACT, ids=[f"{tc.case_id(s)}-{tc.variant(*s)}" for s in tc.EXACT])
def test_gpu_tail_integer_exact(shape):
    E, th, tw, co = shape
    c = tc.integer_case(shape, B=2)
    want64 = tc.tail_f64(c["x"], th, tw, c["conv_w"], c["conv_b"])
    assert np.array_equal(want64, np.rint(want64)) and np.abs(want64).max() < 2 ** 24   # the expectation is exact in f32
    assert np.abs(want64).max() > 64                                                     # and not trivially small
    got = _run(c, th, tw)
    bad = np.argwhere(got.astype(np.float64) != want64)
    assert len(bad) == 0, f"{len(bad)} of {got.size} differ, first (b, co, y, x) = {bad[0].tolist()}"


@pytest.mark.parametrize("shape", [(64, 8, 16, 33), (128, 8, 16, 47)], ids=lambda s: f"{tc.case_id(s)}-{tc.variant(*s)}")
def test_gpu_tail_weight_scale_is_exact(shape):
    """the weights are pre-scaled by a power of two taken from max|w| (split_scale_exp) before the f16 hi / lo split, so
    w 2^k loads the same planes and 2^-k times the inverse scale: with zero bias the output is exactly 2^k times"""
    E, th, tw, co = shape
    c = dict(tc.case(shape, 1, seed=23))
    c["conv_b"] = np.zeros_like(c["conv_b"])
    base = _run(c, th, tw)
    assert np.abs(base).max() > 0.1
    for k in (-20, 20):
        ck = dict(c, conv_w=np.ldexp(c["conv_w"], k).astype(np.float32))
        assert np.array_equal(np.ldexp(ck["conv_w"].astype(np.float64), -k), c["conv_w"])   # the scaling itself is exact
        assert np.array_equal(_run(ck, th, tw), np.ldexp(base, k)), f"k = {k}"


# ------------------------------------------------------------------------------------------ token magnitude
MAG_SHAPES = [(64, 8, 16, 33), (128, 8, 16, 47)]


def _magnitude(oracle, shape, p):
    """zero bias: max|want| then scales with the tokens, and the tolerance (a fraction of it) asks the same at every p"""
    E, th, tw, co = shape
    c = dict(tc.case(shape, 1, seed=24))
    c["x"] = np.ldexp(c["x"], p).astype(np.float32)
    c["conv_b"] = np.zeros_like(c["conv_b"])
    want = oracle.tail_general(c["x"], th, tw, c["conv_w"], c["conv_b"])
    want64 = tc.tail_f64(c["x"], th, tw, c["conv_w"], c["conv_b"])
    got = _run(c, th, tw)
    return got, _report(f"magnitude_p{p:+d}", shape, got, want, want64)


@pytest.mark.parametrize("p", [-6, 0, 12])
@pytest.mark.parametrize("shape", MAG_SHAPES, ids=lambda s: f"{tc.case_id(s)}-{tc.variant(*s)}")
def test_gpu_tail_token_magnitude_in_window(oracle, shape, p):
    got, (e32, e64) = _magnitude(oracle, shape, p)
    assert np.isfinite(got).all()
    assert e32 <= 2e-5 and e64 <= 2e-5


@pytest.mark.parametrize("p", [-10, -12])
@pytest.mark.parametrize("shape", MAG_SHAPES, ids=lambda s: f"{tc.case_id(s)}-{tc.variant(*s)}")
def test_gpu_tail_token_magnitude_below_window_is_finite(oracle, shape, p):
    """below the window the lo plane of the tokens sinks into the f16 subnormals: the result stays finite, its error
    grows as DESIGN.md's table records (no accuracy claim is made there)"""
    got, _ = _magnitude(oracle, shape, p)
    assert np.isfinite(got).all()


# ------------------------------------------------------------------------------------------ refusals and life cycle
def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _load(h, c, E=None, co=None, w=True, b=True):
    """ita_fusion_tail_load with the case's arrays; E / co override what is declared, w / b = False pass NULL"""
    cw, cb = np.ascontiguousarray(c["conv_w"], np.float32), np.ascontiguousarray(c["conv_b"], np.float32)
    return host.lib().ita_fusion_tail_load(h, _ptr(cw) if w else None, _ptr(cb) if b else None,
                                           cw.shape[1] * 4 // 5 if E is None else E, cw.shape[0] if co is None else co)


def _large(h, x, out, batch, th, tw):
    import torch
    rc = host.lib().ita_fusion_tail_large(h, x.data_ptr() if x is not None else None, out.data_ptr() if out is not None else None,
                                          batch, th, tw, C.c_void_p(torch.cuda.current_stream(0).cuda_stream))
    torch.cuda.synchronize()
    return rc


LIFE = (64, 4, 16, 9)


def test_gpu_tail_load_refusals_keep_the_handle_usable():
    import torch
    E, th, tw, co = LIFE
    c = tc.case(LIFE, 1, seed=25)
    ref = torch.from_numpy(_run(c, th, tw)).cuda()
    eng = host.FusionTailLarge(c["conv_w"], c["conv_b"], device=0)
    x = torch.from_numpy(c["x"]).cuda()
    for what, kw, code in [("out_ch = 0", dict(co=0), ITA_ERR_UNSUPPORTED), ("out_ch = 65", dict(co=65), ITA_ERR_UNSUPPORTED),
                           ("E = 0", dict(E=0), ITA_ERR_UNSUPPORTED), ("E = 72", dict(E=72), ITA_ERR_UNSUPPORTED),
                           ("conv_w NULL", dict(w=False), ITA_ERR_INVALID_ARG), ("conv_b NULL", dict(b=False), ITA_ERR_INVALID_ARG)]:
        assert _load(eng._h, c, **kw) == code, what
        assert torch.equal(eng(x, th, tw), ref), f"after the refusal of {what}"
    eng.close()


def test_gpu_tail_large_refusals_keep_the_handle_usable():
    import torch
    E, th, tw, co = LIFE
    c = tc.case(LIFE, 1, seed=25)
    ref = torch.from_numpy(_run(c, th, tw)).cuda()
    x = torch.from_numpy(c["x"]).cuda()
    out = torch.zeros_like(ref)
    h = C.c_void_p()
    assert host.lib().ita_create(C.byref(h), 0) == 0
    try:
        assert _large(h, x, out, 1, th, tw) == ITA_ERR_NO_WEIGHTS           # before any ita_fusion_tail_load
        assert not out.any()
        assert _load(h, c) == 0
        assert _large(h, x, out, 1, th, tw) == 0 and torch.equal(out, ref)
        for what, args, code in [("batch = 65536", (x, out, 65536), ITA_ERR_UNSUPPORTED), ("x NULL", (None, out, 1), ITA_ERR_INVALID_ARG),
                                 ("out NULL", (x, None, 1), ITA_ERR_INVALID_ARG), ("batch = 0", (x, out, 0), ITA_ERR_INVALID_ARG)]:
            out.zero_()
            assert _large(h, *args, th, tw) == code, what
            assert not out.any(), f"{what}: refused, yet something was written"
            assert _large(h, x, out, 1, th, tw) == 0 and torch.equal(out, ref), f"after the refusal of {what}"
    finally:
        host.lib().ita_destroy(h)


def test_gpu_tail_reload_equals_fresh_engine():
    """E = 128 / CO = 48 (up kernel, with its side planes) -> E = 64 / CO = 9 -> E = 128 / CO = 64 on one handle: each
    output is a fresh engine's, bit for bit -- the side planes of the first load must not route the later ones"""
    import torch
    steps = [(128, 8, 16, 48), (64, 8, 16, 9), (128, 8, 16, 64)]
    cases = [tc.case(s, 2, seed=26) for s in steps]
    fresh = [_run(c, s[1], s[2]) for s, c in zip(steps, cases)]
    eng = host.FusionTailLarge(cases[0]["conv_w"], cases[0]["conv_b"], device=0)
    for i, (s, c) in enumerate(zip(steps, cases)):
        if i:
            eng.reload(c["conv_w"], c["conv_b"])
        assert (eng.E, eng.CO) == (s[0], s[3])
        got = eng(torch.from_numpy(c["x"]).cuda(), s[1], s[2]).cpu().numpy()
        assert got.shape == fresh[i].shape and np.array_equal(got, fresh[i]), f"step {i}: {tc.case_id(s)}"
    eng.close()
