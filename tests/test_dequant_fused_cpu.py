"""The fused dequantise form of the two block outputs, out_proj and fc2, on the CPU: the load-time search and proof
(ita_debug_dequant_site, ita_debug_fused_check form 3) on every committed fixture layer, against a re-evaluation in
numpy float32 with an explicit fma.

The form: the site's accumulators start at an int32 pattern C near 0x4B400000 (the base sits in the image's bo / b2), so
an accumulator's pattern is the float C + a;  t = fma(C + a, m, K), K = 1.5 * 2^23 - round(C m);  r = t - 1.5 * 2^23;
code = clamp(r, -128, 127);  d = code * scale.  The definition it is held to is clamp(rne(fl32(a m))).
The fma is evaluated exactly: m = M 2^-s, so (C + a) M + K 2^s is an int64 and t is that over 2^s rounded to nearest,
ties to the even result -- t lies in [2^23, 2^24), where a float32 has ulp 1.  The subtraction and the clamp are then plain
numpy float32 operations."""
import numpy as np

import requant_common as rc
from conftest import golden_files
from drone_oa_iree_vit_accelerator_amd import host, params
from requant_fused_common import DMAX, MAGIC0, amax, candidates, cval, dequant_differs, fma32, in_range, k_of, room

f32 = np.float32
BENCH = "vitlstm_E64_seed0_B2"


def fixture_sites():
    """{fixture.layer.site: (m, dmax)} for out_proj and fc2 of every int8 layer of every committed fixture"""
    out = {}
    for path in golden_files("*.npz"):
        d = params.load_fixture(path)
        name = path.rsplit("/", 1)[-1][:-4]
        for l in range(16):
            if f"attn{l}.q_proj.w_q" not in d or f"ffn{l}.fc1.w_q" not in d:
                continue
            ta, tf = params.attention_tensors(d, f"attn{l}.", l), params.ffn_tensors(d, f"ffn{l}.", l)
            out[f"{name}.{l}.O"] = (f32(ta[f"attn{l}.scal"][rc.SCAL["O"][1]]), room(ta[f"attn{l}.wo"], ta[f"attn{l}.bo"]))
            out[f"{name}.{l}.fc2"] = (f32(tf[f"ffn{l}.scal"][rc.SCAL["fc2"][1]]), room(tf[f"ffn{l}.w2"], tf[f"ffn{l}.b2"]))
    return out


def test_fma32_is_fraction_arithmetic():
    """the explicit fma against Fraction arithmetic, around ties and at random"""
    from fractions import Fraction
    rs = np.random.RandomState(5)
    for m in (f32(0.0013524714158847928), f32(2.0 ** -7), f32(0.0047836629673838615), f32(3.4e-5)):
        fm = Fraction(float(m))
        for C in (host.ACC_BIAS, host.ACC_BIAS - 247716, host.ACC_BIAS + 1):
            K = k_of(m, C, MAGIC0)
            a = np.array(sorted(set(rc.tie_neighbours(m)) | set(int(v) for v in rs.randint(-amax(m), amax(m), 40))), np.int64)
            t = fma32(cval(C) + a, m, K)
            for ai, ti in zip(a, t):
                assert int(ti) == round(Fraction(cval(C) + int(ai)) * fm + K), (m, C, ai)   # half-even on the result


def test_fixture_sites_accepted_equal_refused_differ():
    sites = fixture_sites()
    assert len(sites) >= 8 and f"{BENCH}.0.O" in sites and f"{BENCH}.0.fc2" in sites
    n_ok = n_ref = n_range = 0
    for name, (m, dmax) in sorted(sites.items()):
        got = host.dequant_site(m, dmax)
        if not in_range(m) or dmax < 0:
            assert got is None, name
            n_range += 1
            continue
        cap = min(dmax, DMAX)
        if got is not None:
            C, K = got
            assert abs(C - host.ACC_BIAS) <= cap, (name, C, dmax)            # the base leaves the worst row its room below 2^22
            assert K == int(K) and (1 << 23) <= K < (1 << 24) and K == k_of(m, C, MAGIC0), (name, C, K)
            assert C == next(c for c in candidates(m, cap) if host.fused_check(m, c, dq=True)[0]), name
            bad = dequant_differs(m, C, K)
            assert bad.size == 0, (name, m, C, K, bad[:4])
            n_ok += 1
        else:
            # every candidate of the search was refused: each has an accumulator on which the fused form differs
            for c in candidates(m, cap):
                ok, k = host.fused_check(m, c, dq=True)
                assert not ok and k == k_of(m, c, MAGIC0), (name, c)
                assert dequant_differs(m, c, k).size >= 1, (name, c)
            n_ref += 1
    print(f"{len(sites)} out_proj / fc2 sites of the fixtures: {n_ok} accepted, {n_ref} refused, {n_range} outside the multiplier range")
    assert n_ok >= 2


def test_enumeration_decides_every_candidate_exactly():
    """on the candidates of each fixture site the enumeration accepts exactly when the re-evaluation finds no differing
    accumulator; some are rejected"""
    n_acc = n_rej = 0
    for name, (m, dmax) in sorted(fixture_sites().items()):
        if not in_range(m) or dmax < 0:
            continue
        for c in candidates(m, min(dmax, DMAX)):
            k = k_of(m, c, MAGIC0)
            want = dequant_differs(m, c, k).size == 0
            ok, k2 = host.fused_check(m, c, dq=True)
            assert k2 == k and ok == want, (name, c, want)
            n_acc += want
            n_rej += not want
        # a base whose C m lies far from an integer
        C = candidates(m, min(dmax, DMAX))[0]
        for dlt in (1, 2, 3):
            k = k_of(m, C + dlt, MAGIC0)
            want = dequant_differs(m, C + dlt, k).size == 0
            assert host.fused_check(m, C + dlt, dq=True)[0] == want, (name, dlt)
            n_acc += want
            n_rej += not want
    print(f"candidates: {n_acc} accepted, {n_rej} rejected")
    assert n_acc >= 8 and n_rej >= 8


def test_bench_blob_sites_are_accepted():
    """the seed-0 blob of the default benchmark runs the form at both sites"""
    sites = fixture_sites()
    for s in host.DQ_SITES:
        m, dmax = sites[f"{BENCH}.0.{s}"]
        got = host.dequant_site(m, dmax)
        assert got is not None, s
        assert dequant_differs(m, *got).size == 0


def test_refusals():
    for m in (0.0, -0.001, 1.0, 1.5, float("nan"), float("inf"), 3.2e-5, 1e-30):
        assert host.dequant_site(m) is None, m
        assert host.fused_check(m, host.ACC_BIAS, dq=True)[0] is False, m
    assert host.dequant_site(f32(2.0 ** -7), -1) is None                 # no room at all
    assert host.dequant_site(f32(2.0 ** -7), 0) == (host.ACC_BIAS, float(MAGIC0 - (MAGIC0 >> 7)))   # the default base itself
    assert host.fused_check(f32(0.5), host.ACC_BIAS, dq=True)[0] is False   # K outside [2^23, 2^24)
