"""The fused requantisation form on the CPU: the load-time search and proof (ita_debug_fused_site, ita_debug_fused_check)
against an exact re-computation.

The form: a site's accumulators start at an int32 pattern C near 0x4B400000, so the accumulator's pattern is the float
C + a, and t = fma(C + a, m, K) with K = magic - round(C m) is the only float operation; the low 16 bits of t's pattern
then hold r + 128 and the u8 saturation clamps.  The definition it is held to is the reference's two roundings,
clamp(rne(fl32(a m))) (requant_common).  Everything here is integer arithmetic: m = M 2^-s, so the exact value under
the fma's single rounding is ((C + a) M + K 2^s) / 2^s, an integer K plus N / 2^s, rounded to nearest, ties to the
even RESULT (the parity of K counts).  fma_codes does that on int64 arrays; test_exact_codes_are_fraction_arithmetic
holds it to Fraction arithmetic."""
from fractions import Fraction

import numpy as np
import pytest

import requant_common as rc
from drone_oa_iree_vit_accelerator_amd import host
from requant_fused_common import (DMAX, MAGIC0, MAGIC32K, MAGIC128, amax, candidates, cval, differs, fixture_multipliers, fma_codes,
                                  k_of, ms, proven, ref_codes)

f32 = np.float32


def _sweep():
    fx = fixture_multipliers()
    rs = np.random.RandomState(0)
    sweep = [f32(3e-5 * (1.0 / 3e-5) ** u) for u in rs.uniform(0.0, 1.0, 220)]
    sweep = [m for m in sweep if 3.3e-5 <= m < 1]
    for e in range(1, 15):
        p = f32(2.0 ** -e)
        sweep += [p, np.nextafter(p, f32(0)), np.nextafter(p, f32(1))]
    for m0 in (1.4e-3, 2.3e-3, 4e-3):
        ok, bad = rc.find_multipliers(m0, 6, 6, 3)
        sweep += [m for m, _ in ok + bad]
    sweep += list(fx.values())
    return [np.uint32(b).view(np.float32) for b in sorted({int(f32(m).view(np.uint32)) for m in sweep})], fx


def test_exact_codes_are_fraction_arithmetic():
    """fma_codes against Fraction arithmetic and requant_common's float32 rounding, around ties and at random"""
    rs = np.random.RandomState(3)
    for m in (f32(0.0013524714158847928), f32(2.0 ** -7), f32(0.0047836629673838615), f32(3.4e-5)):
        fm = Fraction(float(m))
        for C in (host.ACC_BIAS, host.ACC_BIAS - 247716, host.ACC_BIAS + 1):
            K = k_of(m, C)
            a = np.array(sorted(set(rc.tie_neighbours(m)) | set(int(v) for v in rs.randint(-amax(m), amax(m), 40))), np.int64)
            got = fma_codes(m, C, K, a)
            for ai, g in zip(a, got):
                exact = Fraction(cval(C) + int(ai)) * fm + K
                t = round(exact)                                   # half-even on the result, as the fma in [2^23, 2^24)
                low = t & 0xFFFF
                assert g == max(0, min(255, low - 65536 if low >= 32768 else low)), (m, C, ai)
            ref = ref_codes(m, a)
            for ai, r in zip(a, ref):
                assert r == rc.clamp8(round(rc.fl32(Fraction(int(ai)) * fm))) + 128, (m, ai)


def test_accepted_sites_equal_the_definition_exactly():
    """every fixture multiplier and the sweep of test_fast_site_ok_equals_the_exact_definition: when the search accepts,
    C and K are within the stated bounds and fma(C + a, m, K) gives the definition's code for EVERY a of the clamp range"""
    sweep, fx = _sweep()
    assert len(sweep) >= 300 and len(fx) >= 100
    n_ok = 0
    for m in sweep:
        got = host.fused_site(m)
        if got is None:
            continue
        C, K = got
        assert abs(C - host.ACC_BIAS) <= DMAX, (m, C)
        assert K == int(K) and (1 << 23) <= K < (1 << 24) and K == k_of(m, C), (m, C, K)
        assert amax(m) + abs(C - host.ACC_BIAS) < 1 << 22
        bad = differs(m, C, K)
        assert bad.size == 0, (m, C, K, bad[:4])
        ok, k2 = host.fused_check(m, C)
        assert ok and k2 == K
        n_ok += 1
    n_fx = sum(host.fused_site(m) is not None for m in fx.values())
    print(f"{len(sweep)} multipliers: {n_ok} accepted; {n_fx} of the {len(fx)} fixture sites")
    assert n_ok > len(sweep) // 4          # the form would be pointless if the search rarely succeeded
    # K = magic - round(C m) stays in [2^23, 2^24) only for m up to about 1/3: nothing above is accepted
    assert all(host.fused_site(m) is None for m in sweep if m > 0.34)


def test_search_takes_the_best_candidates_in_order():
    """the base the search returns is the first of the eight closest-to-integer bases that the enumeration accepts, and
    the candidates' distances are as small as the form needs (C m within about 1e-5 of an integer)"""
    fx = fixture_multipliers()
    for name in sorted(fx)[::7]:
        m = fx[name]
        cs = candidates(m)
        M, s = ms(m)
        eps = [abs(Fraction(cval(C) * M, 1 << s) - round(Fraction(cval(C) * M, 1 << s))) for C in cs]
        assert eps == sorted(eps) and eps[-1] < Fraction(1, 20000), (name, [float(e) for e in eps])
        got = host.fused_site(m)
        assert (got[0] if got else None) == proven(m), name


def test_refusals():
    """m <= 0, m >= 1, non-finite, and below 130 / 4e6, where the enumeration would leave the accumulator range"""
    for m in (0.0, -0.001, -1.0, 1.0, np.nextafter(f32(1), f32(2)), 1.5, 256.0, float("nan"), float("inf"), 3.2e-5, 1e-6, 1e-30):
        assert host.fused_site(m) is None, m
        assert host.fused_check(m, host.ACC_BIAS)[0] is False, m
    # a base from which C + a leaves [2^23, 2^24) within the clamp range
    m = f32(3.4e-5)
    assert host.fused_check(m, host.ACC_BIAS + (1 << 22) - amax(m) + 5)[0] is False
    assert host.fused_check(f32(2.0 ** -7), host.ACC_BIAS - (1 << 22) - 1)[0] is False
    # K outside [2^23, 2^24): m = 0.5 puts round(C m) above magic - 2^23
    assert host.fused_check(f32(0.5), host.ACC_BIAS)[0] is False


@pytest.mark.parametrize("logits", [False, True], ids=["codes", "logits"])
def test_enumeration_rejects_a_base_that_differs(logits):
    """for accepted (m, C): neighbouring bases whose C m lies far from an integer make some accumulator round
    differently; the enumeration must reject exactly those (decided here by the exact re-computation)"""
    fx = fixture_multipliers()
    magic = MAGIC32K if logits else MAGIC128
    n_rej = n_acc = 0
    for name in ("vitlstm_E64_seed0_B2.attn0.Q", "vitlstm_E64_seed0_B2.attn0.L", "blocks_E128_seed0_B1.attn0.C"):
        m = fx[name]
        C, _ = host.fused_site(m)
        assert differs(m, C, k_of(m, C, magic), logits).size == 0
        assert host.fused_check(m, C, logits)[0]
        for d in range(1, 25):
            C2 = C + d
            want = differs(m, C2, k_of(m, C2, magic), logits).size == 0
            ok, k = host.fused_check(m, C2, logits)
            assert k == k_of(m, C2, magic)
            assert ok == want, (name, C2, want)
            n_rej += not want
            n_acc += want
    print(f"{n_rej} neighbouring bases rejected, {n_acc} accepted")
    assert n_rej >= 30


def test_relu_form_enumeration_is_exact():
    """fc1's fused ReLU form (K = 1.5 * 2^23 - round(C m), codes clamped to [0, 127]): on every fixture's fc1 multiplier the
    enumeration accepts a candidate exactly when the exact re-computation finds no differing accumulator, negative ones
    included (they must saturate to 0)"""
    fx = fixture_multipliers()
    n_ok = n_bad = 0
    for name in sorted(k for k in fx if k.endswith(".fc1")):
        m = fx[name]
        for C in candidates(m):
            K = k_of(m, C, MAGIC0)
            want = differs(m, C, K, relu=True).size == 0
            ok, k = host.fused_check(m, C, relu=True)
            assert k == K and ok == want, (name, C, want)
            n_ok += want
            n_bad += not want
    print(f"fc1 candidates: {n_ok} accepted, {n_bad} rejected")
    assert n_ok >= 8 and n_bad >= 8
    assert proven(fx["vitlstm_E64_seed0_B2.ffn0.fc1"], relu=True) is not None      # the bench blob's fc1 runs it


def test_bench_blob_sites_are_accepted():
    """the seed-0 blob of the default benchmark: all five fused sites of its encoder layer are accepted, and its six
    sites pass the single-rounding proof too, so the layer runs the fused instantiation (asserted on the engine in
    test_gpu_requant_fused.py)"""
    fx = fixture_multipliers()
    for s in rc.ATTN_SITES:
        assert host.fast_site_ok(fx[f"vitlstm_E64_seed0_B2.attn0.{s}"]), s
    for s in host.FUSED_SITES:
        assert host.fused_site(fx[f"vitlstm_E64_seed0_B2.attn0.{s}"]) is not None, s
    # and a fixture with refused sites, which keeps the other forms
    assert any(host.fused_site(fx[f"blocks_E64_seed2_B1.attn0.{s}"]) is None for s in host.FUSED_SITES)
