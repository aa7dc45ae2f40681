"""The u8 tokenizer's integer conv at per-channel scales and on 0 / 255 frames, on the CPU: the crafted sets hold what they
claim, an independent numpy model of the kernel's signed-byte form equals the oracle bit for bit, both oracle entries stay
within 1e-5 of float64, three table mutations break that bound on the crafted sets (and one of them does not on the stock
weights, which is why the stock tests cannot see it), and one-hot frames touch their footprint only.
tests/test_gpu_tokenizer_edges.py holds the kernels to the oracle on the same sets and frames."""
import ctypes

import numpy as np
import pytest

import tokenizer_edges_common as tc

CASES = [(E, s) for E in tc.ES for s in tc.SETS]


def _quant_of(E, name):
    return tc.quantise(tc.weights(E, name)[0])


@pytest.mark.parametrize("E", tc.ES)
def test_stock_weights_share_one_exponent(E):
    """the gap: every channel of the stock seed-0 weights has e_c = 24, and synth.frames holds no pixel code 255"""
    from drone_oa_iree_vit_accelerator_amd import synth
    _, e, _ = _quant_of(E, "stock")
    assert set(e.tolist()) == {24}
    img = synth.frames(0, 64)["img_u8"]
    assert (img == 255).sum() == 0


@pytest.mark.parametrize("E", tc.ES)
def test_sets_hold_their_edges(E):
    n = {s: len(set(_quant_of(E, s)[1].tolist())) for s in tc.SETS}
    print(f"E = {E}: distinct e_c per set {n}")
    assert n["graded"] >= 7 and n["wide"] >= 16 and n["digits"] >= 5
    # graded: the channels of one 16-tile (E/4 kq + 4 ct + i) and adjacent channels differ
    _, e, _ = _quant_of(E, "graded")
    assert (e[0::2] != e[1::2]).all()
    for ct in range(E // 16):
        tile = [E // 4 * kq + 4 * ct + i for kq in range(4) for i in range(4)]
        assert len(set(e[tile].tolist())) >= 5
    # wide: weights above 1, the dead channel, the underflowing scale, the power of two, Wq = +-2^22 by rounding up
    cw = tc.weights(E, "wide")[0]
    wq, e, s = _quant_of(E, "wide")
    assert (np.abs(cw) >= 1).any()
    assert e[tc.DEAD] == 0 and (wq[tc.DEAD] == 0).all() and s[tc.DEAD] == np.float32(1) / np.float32(65280)
    assert s[tc.TINY] == 0 and e[tc.TINY] == 161 and (wq[tc.TINY] == 1 << 21).all()
    assert np.abs(wq[tc.POW2]).max() == 1 << 21 and np.frexp(np.abs(cw[tc.POW2]).max())[0] == 0.5
    assert wq[tc.UP_POS].max() == 1 << 22 and wq[tc.UP_NEG].min() == -(1 << 22)
    assert np.abs(wq).max() == 1 << 22
    w0, w1, w2 = tc.byte_planes(wq)
    assert w2.max() == 64 and w2.min() == -64              # +-2^22 = 64 * 65536: the top digit's extreme
    # taps: one weight per channel, every tap (the 49 slots of the A fragment image) named by some channel
    cw = tc.weights(E, "taps")[0]
    assert ((cw != 0).sum(1) == 1).all() and set(np.nonzero(cw)[1].tolist()) == set(range(49))
    assert (np.abs(cw[np.arange(E), np.arange(E) % 49]) == 1 + np.arange(E) / 64).all()
    # digits: exactly the integers, every channel with every plane at both ends and both carries
    ints, e_want = tc.digit_integers(E)
    wq, e, _ = _quant_of(E, "digits")
    assert np.array_equal(wq, ints) and np.array_equal(e, e_want)
    assert np.array_equal(np.ldexp(tc.weights(E, "digits")[0].astype(np.float64), e[:, None]), ints)
    assert (np.abs((1 << 22) - np.abs(wq[:, 0])) <= 3).all() and (np.abs(wq).max(1) == np.abs(wq[:, 0:2]).max(1)).all()
    w0, w1, w2 = tc.byte_planes(wq)
    for w in (w0, w1):
        assert (w.min(1) == -128).all() and (w.max(1) == 127).all()
    assert (w2.min(1) == -64).all() and (w2.max(1) == 64).all()
    r1 = (wq - w0) >> 8
    assert ((r1 != wq >> 8).any(1)).all() and (((r1 - w1) >> 8 != r1 >> 8).any(1)).all()     # both carries fire
    assert np.array_equal(65536 * w2 + 256 * w1 + w0, wq)


def test_frames_hold_their_edges():
    f = tc.frames()
    assert f.dtype == np.uint8 and f.shape == (len(tc.FRAME_NAMES), 60, 90)
    assert (f[tc.ZEROS] == 0).all() and (f[tc.FULL] == 255).all()
    assert set(np.unique(f[2]).tolist()) == {0, 255} and set(np.unique(f[4]).tolist()) == {0, 1, 254, 255}
    assert len(np.unique(f[3])) == 256
    for i, (r, c) in enumerate(tc.ONE_HOT):
        assert f[tc.FIRST_HOT + i].sum() == 255 and f[tc.FIRST_HOT + i, r, c] == 255
    t = tc.blended_taps(f)
    lo, hi = t & 255, t >> 8
    assert t.max() == 65280 and t.min() == 0                # B256 = 65280: a1 = 255, a0 = 0
    assert (lo == 255).any() and ((hi == 255) & (lo == 0)).any()
    assert (tc.blended_taps(f[tc.FULL])[0, 5 * 16 + 7] == 65280).all()     # an interior token of the saturated frame
    x = tc.frames_f32(f)
    assert x.dtype == np.float32 and x.max() == 1 and x[4].min() == 0


@pytest.mark.parametrize("E,name", CASES + [(64, "stock"), (128, "stock")])
def test_oracle_quantisation_is_the_numpy_one(oracle, E, name):
    cw = tc.weights(E, name)[0]
    wq, sc = np.empty((E, 49), np.int32), np.empty(E, np.float32)
    fn = oracle.lib().ita_oracle_tok_quant_weights
    fn.restype = None
    fn(cw.ctypes.data_as(ctypes.c_void_p), ctypes.c_int(E), wq.ctypes.data_as(ctypes.c_void_p), sc.ctypes.data_as(ctypes.c_void_p))
    nq, _, ns = tc.quantise(cw)
    assert np.array_equal(wq, nq) and np.array_equal(sc.view(np.uint32), ns.view(np.uint32))


def test_fma32_rounds_once():
    """the model's float32 fma against exact rational arithmetic, on operands built to double-round"""
    from fractions import Fraction
    rs = np.random.RandomState(3)
    a = rs.standard_normal(4000).astype(np.float32)
    b = rs.standard_normal(4000).astype(np.float32)
    c = (rs.standard_normal(4000) * np.exp(rs.uniform(-20, 20, 4000))).astype(np.float32)
    # c = a float32 tie point minus a * b up to float64 rounding: a * b + c lands next to a tie of the float32 grid
    x = rs.standard_normal(2000).astype(np.float32)
    tie = x.astype(np.float64) + np.spacing(x).astype(np.float64) / 2
    c[:2000] = (tie - a[:2000].astype(np.float64) * b[:2000].astype(np.float64)).astype(np.float32)
    got = tc.fma32(a, b, c)
    for i in range(len(a)):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo = np.float32(float(exact))                       # Fraction -> float is correctly rounded, but to float64 first
        cands = {lo, np.nextafter(lo, np.float32(np.inf)), np.nextafter(lo, np.float32(-np.inf))}
        best = min(abs(Fraction(float(x)) - exact) for x in cands)
        near = [x for x in cands if abs(Fraction(float(x)) - exact) == best]
        want = near[0] if len(near) == 1 else [x for x in near if (np.float32(x).view(np.uint32) & 1) == 0][0]
        assert got[i] == want, (i, a[i], b[i], c[i])


@pytest.mark.parametrize("E,name", CASES)
def test_model_equals_oracle(oracle, E, name):
    """the signed-byte / I0 / I2 form of the kernel and its table is the definition: bit for bit on every frame"""
    cw, cb, lw, lb = tc.weights(E, name)
    f = tc.frames()
    pre = tc.tok_u8_model(f, cw, cb)
    got = oracle.add_ln(pre, np.zeros_like(pre), lw, lb)
    want = oracle.tokenizer(f, cw, cb, lw, lb)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


_ORACLE = {}


def _oracle_tokens(oracle, E, name):
    """(u8 entry, f32 entry) of the oracle on every frame, computed once per (E, set)"""
    if (E, name) not in _ORACLE:
        f = tc.frames()
        _ORACLE[E, name] = tuple(_ro(oracle.tokenizer(x, *tc.weights(E, name))) for x in (f, tc.frames_f32(f)))
    return _ORACLE[E, name]


def _ro(a):
    a.setflags(write=False)
    return a


@pytest.mark.parametrize("E,name", CASES)
def test_oracle_within_1e_5_of_float64(oracle, E, name):
    """both oracle entries against the float64 map from the exact codes / 255; the GPU equals them bit for bit
    (test_gpu_tokenizer_edges.py), so this bound holds for the kernels too"""
    want = tc.tokens_f64_of(E, name)
    u8, f32 = _oracle_tokens(oracle, E, name)
    eu = np.abs(u8 - want).reshape(len(want), -1).max(1)
    ef = np.abs(f32 - want).reshape(len(want), -1).max(1)
    print(f"E = {E} {name}: max |oracle - f64| u8 {eu.max():.2e} (frame {tc.FRAME_NAMES[eu.argmax()]}), "
          f"f32 {ef.max():.2e} (frame {tc.FRAME_NAMES[ef.argmax()]}); max |token| {np.abs(want).max():.2f}")
    assert eu.max() <= tc.BOUND and ef.max() <= tc.BOUND


MUTATIONS = (("swap_scale", "graded"), ("i2_without_w1", "digits"), ("no_carry", "digits"))


@pytest.mark.parametrize("E", tc.ES)
def test_mutations_break_the_bound(oracle, E):
    """a table that takes channel c ^ 1's scale, an I2 without its sum of w1, or digits without their carry leaves the
    float64 bound on the crafted set named for it -- and the first does NOT on the stock weights (one e_c for all
    channels: the stock fixtures are blind to it)"""
    f = tc.frames()

    def err(name, **mutation):
        cw, cb, lw, lb = tc.weights(E, name)
        pre = tc.tok_u8_model(f, cw, cb, **mutation)
        return float(np.abs(oracle.add_ln(pre, np.zeros_like(pre), lw, lb) - tc.tokens_f64_of(E, name)).max())

    for name in tc.SETS + ("stock",):
        assert err(name) <= tc.BOUND                        # the model itself is inside the bound everywhere
    for mutation, expect in MUTATIONS:
        errs = {name: err(name, **{mutation: True}) for name in tc.SETS + ("stock",)}
        print(f"E = {E} {mutation}: max |tokens - f64| " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
        assert errs[expect] > tc.BOUND, (mutation, errs)
    assert err("stock", swap_scale=True) <= tc.BOUND


@pytest.mark.parametrize("E,name", [(E, s) for E in tc.ES for s in ("graded", "taps")])
def test_one_hot_frames_touch_their_footprint_only(oracle, E, name):
    for tok in _oracle_tokens(oracle, E, name):
        bits = tok.view(np.uint32)
        for i, (r, c) in enumerate(tc.ONE_HOT):
            fp = tc.footprint(r, c)
            assert fp.any() and not fp.all()
            assert np.array_equal(bits[tc.FIRST_HOT + i][~fp], bits[tc.ZEROS][~fp]), (r, c)
            assert (bits[tc.FIRST_HOT + i][fp] != bits[tc.ZEROS][fp]).any(), (r, c)
            for (r2, c2) in tc.ALIASES.get((r, c), ()):
                # the frame byte of (r, c) is also the byte a window without its column masks would read as (r2, c2)
                assert r * 90 + c == r2 * 90 + c2
                alias = tc.reads(r2, c2)
                assert alias.any() == (c2 != 92)           # x0 <= 43: no tap lies over image column 92 (window column 95)
                assert not (alias & fp).any()
                assert np.array_equal(bits[tc.FIRST_HOT + i][alias], bits[tc.ZEROS][alias]), (r, c, r2, c2)


def test_footprint_is_the_support_of_the_float64_map():
    """footprint against the map itself: the tokens a one-hot frame moves in float64 (unit weights: no cancellation)"""
    E = 64
    _, cb, lw, lb = tc.stock(E)
    cw = np.ones((E, 49), np.float32) * np.arange(1, E + 1, dtype=np.float32)[:, None]
    f = tc.frames()
    t = tc.tokens_f64(f, cw, cb, lw, lb)
    for i, (r, c) in enumerate(tc.ONE_HOT):
        moved = (t[tc.FIRST_HOT + i] != t[tc.ZEROS]).any(-1)
        assert np.array_equal(moved, tc.footprint(r, c)), (r, c)
