"""Shared by test_requant_cpu.py and test_gpu_requant_edges.py: the requantisation step in exact arithmetic, and blobs
crafted so that chosen int32 accumulators occur at a chosen site.

The step is q = clamp(rne(fl32(f32(acc) * m)), -128, 127): TWO roundings (the product to float32, then to an integer).
A fused multiply-add rounds the exact product ONCE.  single_vs_double(m) lists, in integer / Fraction arithmetic, the
accumulators on which the two disagree after the clamp; that is the definition ita_load_weights' proof (fast_site_ok)
is held to, and those accumulators are what the crafted blobs put at a site.

Sites: Q, K, V, L (matmul1), C (matmul2), O of the attention block, fc1 and fc2 of the FFN.
"""
import functools
import math
from fractions import Fraction

import numpy as np

from conftest import golden_files
from drone_oa_iree_vit_accelerator_amd import mha_heads_ref as ref
from drone_oa_iree_vit_accelerator_amd import params, synth

f32 = np.float32
ATTN_SITES = ("Q", "K", "V", "L", "C", "O")          # bit order of the engine's fast_sites mask
FFN_SITES = ("fc1", "fc2")
SITES = ATTN_SITES + FFN_SITES
MHA_TAPS = ("x_q", "Q", "K", "V", "logits", "probs", "ctx", "out_q")
LINEAR = {"Q": ("attn0.wq", "attn0.bq"), "K": ("attn0.wk", "attn0.bk"), "V": ("attn0.wv", "attn0.bv"),
          "O": ("attn0.wo", "attn0.bo"), "fc1": ("ffn0.w1", "ffn0.b1"), "fc2": ("ffn0.w2", "ffn0.b2")}
SCAL = {"Q": ("attn0.scal", ref.MQ), "K": ("attn0.scal", ref.MK), "V": ("attn0.scal", ref.MV), "L": ("attn0.scal", ref.ML),
        "C": ("attn0.scal", ref.MC), "O": ("attn0.scal", ref.MO), "fc1": ("ffn0.scal", ref.M1), "fc2": ("ffn0.scal", ref.M2)}
TIE_KS = (-129, -128, -1, 0, 126, 127)               # the ties k + 0.5 at the clamp's two ends and at zero
FIXTURE = {64: "blocks_E64_seed2_B1.npz", 128: "blocks_E128_seed0_B1.npz"}
C_HOT = 64               # site C: 64 keys with the probability 2 and 64 with 1 (rounding_case), codes in [-127, 127]
C_MAX = 3 * C_HOT * 127


def requant_single(acc, mult):
    """requantisation with ONE rounding, clip(rint(acc * f32(mult) exactly)): a 24-bit accumulator times a 24-bit
    multiplier is exact in float64.  What a fused multiply-add computes: the wrong answer, unless fast_site_ok admits mult"""
    assert np.abs(acc).max(initial=0) < (1 << 24)
    return np.clip(np.rint(acc.astype(np.float64) * np.float64(f32(mult))), -128, 127).astype(np.int8)


def once_at(*sites):
    """the rq hook of mha_heads_ref.mha / ffn that rounds once at these sites and as the block does elsewhere"""
    return lambda site, acc, m: (requant_single if site in sites else ref.requant)(acc, m)


# ---- exact arithmetic ------------------------------------------------------------------------------------------
def fl32(x: Fraction) -> Fraction:
    """x rounded to the nearest float32, ties to even (normal range), as an exact Fraction"""
    if x == 0:
        return Fraction(0)
    s, a = (-1 if x < 0 else 1), abs(Fraction(x))
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    assert Fraction(2) ** e <= a < Fraction(2) ** (e + 1) and -126 <= e < 127
    ulp = Fraction(2) ** (e - 23)
    return s * round(a / ulp) * ulp          # round(Fraction) is round-half-even: the parity is the mantissa's


def clamp8(r: int) -> int:
    return max(-128, min(127, int(r)))


def ulp32(v: Fraction) -> Fraction:
    return Fraction(2) ** (math.floor(math.log2(abs(v))) - 23)


@functools.lru_cache(maxsize=None)
def _single_vs_double(mbits: int):
    m = Fraction(float(np.uint32(mbits).view(np.float32)))
    A = int(Fraction(130) / m) + 2
    out = set()
    # the two can differ only where fl32(a m) lies exactly on a tie k + 0.5 while a m itself does not (rounding to
    # float32 is monotone and every k + 0.5 of this range is a float32): visit the few a around each (k + 0.5) / m
    for k in range(-int(130 + 3 * m) - 3, int(130 + 3 * m) + 3):
        v = Fraction(2 * k + 1, 2)
        u = 2 * ulp32(v)
        lo, hi = sorted(((v - u) / m, (v + u) / m))
        for a in range(math.floor(lo), math.ceil(hi) + 1):
            if abs(a) > A or fl32(a * m) != v:
                continue
            if clamp8(round(a * m)) != clamp8(round(v)):
                out.add(a)
    return tuple(sorted(out))


def single_vs_double(m) -> list:
    """every accumulator a, |a| <= 130 / m + 2, with clamp(rne(a m exactly)) != clamp(rne(fl32(a m))); m a float32 in (0, 1)"""
    m = f32(m)
    assert 0 < m < 1
    return list(_single_vs_double(int(m.view(np.uint32))))


@functools.lru_cache(maxsize=None)
def _find_multipliers(m0bits, n_pass, n_fail, seed, max_abs, lo):
    m0 = float(np.uint32(m0bits).view(np.float32))
    rs = np.random.RandomState(seed)
    ok, bad = [], []
    for _ in range(4000):
        if len(ok) >= n_pass and len(bad) >= n_fail:
            break
        m = f32(m0 * 2.0 ** rs.uniform(-1.0, 1.0))
        if lo is not None and m < lo:
            continue
        diff = single_vs_double(m)
        if not diff and len(ok) < n_pass:
            ok.append((m, ()))
        elif diff and len(bad) < n_fail and (max_abs is None or max(abs(a) for a in diff) <= max_abs):
            bad.append((m, tuple(diff)))
    assert len(ok) == n_pass and len(bad) == n_fail, (m0, len(ok), len(bad))
    return tuple(ok), tuple(bad)


def find_multipliers(m0, n_pass, n_fail, seed, max_abs=None, lo=None):
    """seeded float32 multipliers in [m0 / 2, 2 m0] -> (n_pass of them with an empty single_vs_double, n_fail with a
    non-empty one), each as (m, its differing accumulators); max_abs: only failing ones whose accumulators are within it;
    lo: only multipliers of at least lo"""
    return _find_multipliers(int(f32(m0).view(np.uint32)), n_pass, n_fail, seed, max_abs, lo)


def tie_neighbours(m, max_abs=None) -> list:
    """the two accumulators on either side of every tie (k + 0.5) / m, k in TIE_KS, and their negatives"""
    fm, out = Fraction(float(f32(m))), set()
    for k in TIE_KS:
        q = Fraction(2 * k + 1, 2) / fm
        for a in (math.floor(q), math.ceil(q)):
            out.update((a, -a))
    return sorted(a for a in out if max_abs is None or abs(a) <= max_abs)


def targets(m, diff, max_abs=None) -> list:
    """what a rounding case must put at its site: a*, a* +- 1 for every differing a* (they come in +- pairs), and the
    neighbours of the ties; most important first"""
    out = []
    for a in list(diff) + [a + s for a in diff for s in (-1, 1)] + tie_neighbours(m, max_abs):
        if a not in out and (max_abs is None or abs(a) <= max_abs):
            out.append(a)
    return out


# ---- fixtures --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def base(E):
    """(block tensors with the four LayerNorm vectors and nothing else of the float graph, the fixture's token frame):
    such a blob gets its whole-layer stream image, and no decoder fold is built at load; read-only"""
    d = params.load_fixture(golden_files(FIXTURE[E])[0])
    t = {**params.attention_tensors(d, "attn0.", 0), **params.ffn_tensors(d, "ffn0.", 0)}
    ft = params.float_tensors(synth.float_params(int(d["meta.seed"]), E=E, tail=(E == 64)))
    for k in ("norm1_0.w", "norm1_0.b", "norm2_0.w", "norm2_0.b"):
        t[k] = ft[k]
    return t, np.ascontiguousarray(d["s0.attn0.x_q.in"][:1], np.float32)


def multiplier_of(t, site):
    name, idx = SCAL[site]
    return f32(t[name][idx])


def set_multiplier(t, site, m):
    name, idx = SCAL[site]
    t[name][idx] = f32(m)


@functools.lru_cache(maxsize=None)
def passing(E):
    """one admitted multiplier near the fixture's own for each of the six attention sites"""
    t, _ = base(E)
    return {s: find_multipliers(multiplier_of(t, s), 1, 0, 100 + i)[0][0][0] for i, s in enumerate(ATTN_SITES)}


def pow2_near(m):
    return f32(2.0 ** round(math.log2(float(m))))


@functools.lru_cache(maxsize=None)
def rounding_multipliers(E, site):
    """the cases of one site: [(kind, m, differing accumulators)]: two refused, two admitted, one power of two"""
    t, _ = base(E)
    m0 = multiplier_of(t, site)
    if site == "C":      # its construction reaches |a| <= C_MAX: the part of [m0 / 2, 2 m0] where every tie neighbour fits
        lo = f32(130.0 / (C_MAX - 2))
        ok, bad = find_multipliers(m0, 2, 2, 7, max_abs=C_MAX - 1, lo=lo)
        p2 = f32(2.0 ** -7)
        assert lo < 2 * m0 and m0 / 2 <= p2 <= 2 * m0
    else:
        ok, bad = find_multipliers(m0, 2, 2, 7)
        p2 = pow2_near(m0)
    assert single_vs_double(p2) == []
    return [("refused", m, d) for m, d in bad] + [("admitted", m, d) for m, d in ok] + [("pow2", p2, ())]


def rounding_ids():
    return [(E, s, j) for E in (64, 128) for s in SITES for j in range(5)]


def spread(n, rows):
    """n distinct channels of `rows`, strided so that they fall on different MFMA tiles, lanes and registers"""
    step = next(s for s in (7, 5, 3, 1) if math.gcd(s, rows) == 1)
    assert n <= rows
    return [(3 + j * step) % rows for j in range(n)]


def codes_to_float(codes, t):
    """float tokens that the attention block's quantiser maps back to these int8 codes"""
    x = codes.astype(np.float32) / t["attn0.scal"][ref.INV_SX]
    assert np.array_equal(ref.quantize(x, t["attn0.scal"][ref.INV_SX]), codes.astype(np.int8))
    return x


def split_sum(a, n, lim=127):
    """n integers in [-lim, lim] that sum to a"""
    assert abs(a) <= n * lim
    s, a = (-1 if a < 0 else 1), abs(a)
    q, r = divmod(a, n)
    return s * np.array([q + 1] * r + [q] * (n - r), np.int64)


class Case:
    """one crafted blob: tensors t, head count H, float frames x (B, 128, E), the site and the accumulators it must show"""

    def __init__(self, name, E, site, m, kind, diff, t, x, want, H=1, long_idx=(0, 1)):
        self.name, self.E, self.site, self.m, self.kind, self.diff = name, E, site, f32(m), kind, tuple(diff)
        self.t, self.x, self.want, self.H, self.long_idx = t, x, list(want), H, list(long_idx)

    def blob(self):
        return params.pack_blob(self.t, E=self.E, H=self.H, has_tail=False)

    @functools.lru_cache(maxsize=None)
    def expect(self):
        """the definition on this case: dict of mha / ffn (out, taps, accumulators), encoder layer x2, long forms"""
        from oracle import oracle
        oracle.build()
        t, x = self.t, self.x
        out = dict(mha=ref.mha(x, t, self.H, taps=True), ffn=ref.ffn(x, t, taps=True))
        x1 = oracle.add_ln(x, out["mha"][0], t["norm1_0.w"], t["norm1_0.b"])
        f1 = ref.ffn(x1, t, taps=True)
        out["ffn_x1"] = f1
        out["x2"] = oracle.add_ln(x1, f1[0], t["norm2_0.w"], t["norm2_0.b"])
        xl = np.ascontiguousarray(x[self.long_idx].reshape(1, 256, self.E))   # S = 256, B = 1: two frames as one row
        out["x_long"] = xl
        out["long"] = ref.mha(xl, t, self.H, taps=True)
        return out

    def present(self, acc):
        """how many of the wanted accumulators occur in acc"""
        return int(np.isin(np.array(self.want, np.int64), acc).sum())


def _frames(E):
    t, xf = base(E)
    rs = np.random.RandomState(11)
    return [xf[0], (-0.5 * xf[0][::-1] + 0.01 * rs.standard_normal(xf[0].shape)).astype(np.float32)]


@functools.lru_cache(maxsize=None)
def rounding_case(E, site, j, H=1):
    """Rounding case j of a site (see rounding_multipliers).  Every other attention site gets an admitted multiplier,
    so the engine's mask is all six bits, less this site's where it is refused.

    Linear sites: up to 40 spread output channels get a zero weight row and a wanted accumulator as their bias, so the
    channel's accumulator IS that value on every token of every frame, the fixture's own included.
    C: a crafted frame is non-zero only in features whose columns of Wq are zero; Q is 64 on one channel by its bias and
    0 elsewhere, K = x_q there (2 on the first 64 keys, 0 on the others), ml = 2^-7: the logits are 1 and 0 on every row,
    the probabilities 2 and 1.  V = x_q on one channel per wanted accumulator (one-hot rows of 64, mv = 2^-6), so that
    channel's accumulator is 2 (sum of the first 64 codes) + (sum of the others) on every query row.  A last frame with
    K = -16 has the logit -8 against those rows, 9 below their maximum: probability 0, so the crafted frame and this
    one as one row of 256 tokens hold the same accumulators (the long form).
    L: a crafted frame is non-zero only in 9 features whose columns of Wq are zero; Q is (127 x 8, 1, 0 ...) by its
    biases, K = x_q on those 9 channels, so key s has the accumulator 127 (k_0 + .. + k_7) + k_8 on every query row; one such
    frame per band of nearby logit values."""
    kind, m, diff = rounding_multipliers(E, site)[j]
    t0, _ = base(E)
    t = {k: v.copy() for k, v in t0.items()}
    for s, mp in passing(E).items():
        set_multiplier(t, s, mp)
    set_multiplier(t, site, m)
    frames = _frames(E)
    if site in LINEAR:
        want = targets(m, diff)
        assert len(want) <= 40
        wn, bn = LINEAR[site]
        rows = spread(len(want), t[wn].shape[0])
        t[wn][rows] = 0
        t[bn][rows] = np.array(want, np.int32)
    elif site == "C":
        want = targets(m, diff)
        nf, fk, c0 = len(want), 4 + len(want), 0
        feats = list(range(4, 4 + nf))
        assert nf <= 30 and max(abs(a) for a in want) <= C_MAX
        for s_, m_ in (("V", 2.0 ** -6), ("K", 2.0 ** -6), ("L", 2.0 ** -7)):
            set_multiplier(t, s_, f32(m_))
        t["attn0.wq"][:, feats + [fk]] = 0
        t["attn0.wq"][c0], t["attn0.bq"][:] = 0, 0
        t["attn0.bq"][c0] = math.ceil(64.0 / float(multiplier_of(t, "Q")))      # Q = 64 on channel c0, 0 elsewhere
        t["attn0.wk"][c0], t["attn0.bk"][c0] = 0, 0
        t["attn0.wk"][c0, fk] = 64
        chans = spread(nf, 192)
        t["attn0.wv"][chans] = 0
        t["attn0.bv"][chans] = 0
        for c, f in zip(chans, feats):
            t["attn0.wv"][c, f] = 64
        codes = np.zeros((128, E), np.int64)
        codes[:C_HOT, fk] = 2
        for f, a in zip(feats, want):
            h = int(a / 3)
            rs = np.random.RandomState(abs(a) % 1000)
            codes[:C_HOT, f] = rs.permutation(split_sum(h, C_HOT))
            codes[C_HOT:, f] = rs.permutation(split_sum(a - 2 * h, 128 - C_HOT))
        cold = np.zeros((128, E), np.int64)
        cold[:, fk] = -16
        frames += [codes_to_float(codes, t), codes_to_float(cold, t)]
    else:
        want = targets(m, diff)
        nq = 8
        feats = list(range(4, 4 + nq + 1))
        assert max(abs(a) for a in want) <= 127 * 127 * nq + 127
        set_multiplier(t, "K", f32(2.0 ** -6))
        t["attn0.wq"][:, feats] = 0
        t["attn0.wq"][:nq + 1] = 0
        t["attn0.bq"][:] = 0
        t["attn0.bq"][:nq] = 1 << 20                                     # saturates: Q = 127
        t["attn0.bq"][nq] = int(round(1.0 / float(multiplier_of(t, "Q"))))   # Q = 1
        t["attn0.wk"][:nq + 1] = 0
        t["attn0.bk"][:nq + 1] = 0
        for c, f in enumerate(feats):
            t["attn0.wk"][c, f] = 64
        # one crafted frame per band of logit values: a logit more than 8 below its row's maximum has the probability 0
        # whatever it rounds to, so the wanted accumulators of a frame lie within 6 codes of each other
        frames = frames[:1]
        bands, fm = [], Fraction(float(m))
        for a in sorted(want, key=lambda a: (a != want[0], a)):          # the first wanted one opens the first band
            v = Fraction(a) * fm
            band = next((b for b in bands if abs(Fraction(b[0]) * fm - v) <= 6), None)
            if band is None:
                bands.append(band := [])
            band.append(a)
        for band in bands:
            codes = np.zeros((128, E), np.int64)
            for s in range(128):
                a = band[s % len(band)]
                sg, (n, r) = (-1 if a < 0 else 1), divmod(abs(a), 127)
                codes[s, feats[:nq]] = sg * split_sum(n, nq)
                codes[s, feats[nq]] = sg * r
            frames.append(codes_to_float(codes, t))
    x = np.ascontiguousarray(np.stack(frames), np.float32)
    assert x.shape[0] <= 8
    return Case(f"E{E}-{site}-{kind}{j % 2 if kind != 'pow2' else ''}", E, site, m, kind, diff, t, x, want, H,
                long_idx={"C": (2, 3), "L": (1, 1)}.get(site, (0, 1)))   # (L: the band of the first differing accumulator, twice)


def expected_mask(case):
    """the fast_sites mask the engine must report for a rounding case"""
    full = 63
    if case.site in ATTN_SITES and case.kind == "refused":
        return full & ~(1 << ATTN_SITES.index(case.site))
    return full


def site_accumulators(case, exp, route="mha"):
    """the accumulators of the case's site on a route of Case.expect()"""
    if case.site in ATTN_SITES:
        return exp[route][2][case.site]
    return exp["ffn" if route == "mha" else route][2][case.site]


# ---- the edges of stream_range_ok ------------------------------------------------------------------------------
ACC_BOUND = 1 << 22        # sum |w| * 128 + |b| must stay BELOW this (the accumulator as the float 1.5 * 2^23 + sum)
TRAVEL = 32000.0           # and (sum |w| * 128 + |b|) * m below this (the 16-bit travel format)
TRAVEL_SUM = 1 << 21       # the row sum of the travel cases: 32000 / 2^21 = 125 * 2^-13 is a float32
RANGE_KINDS = ("acc_in", "acc_out", "travel_in", "travel_out")
L_WORST = 192 * 128 * 128


def range_ids():
    return [(E, s, k) for E in (64, 128) for s in LINEAR for k in RANGE_KINDS] + \
           [(E, "L", k) for E in (64, 128) for k in RANGE_KINDS[2:]]


def travel_multipliers(total):
    """(the largest float32 m with total * m < 32000, the smallest with total * m >= 32000), in exact arithmetic"""
    m = f32(TRAVEL / total)
    while Fraction(float(m)) * total >= Fraction(32000):
        m = np.nextafter(m, f32(0))
    while Fraction(float(np.nextafter(m, f32(1)))) * total < Fraction(32000):
        m = np.nextafter(m, f32(1))
    return m, np.nextafter(m, f32(1))


@functools.lru_cache(maxsize=None)
def range_case(E, site, kind):
    """A blob with one weight row pair at an edge of stream_range_ok, and frames that drive the accumulator to it.

    Linear site, rows 5 and N - 3: w = -127 with b = +top, and w = +127 with b = -top (fc2: the other way round), where 127 * 128 * nnz + top is
    2^22 - 1 (acc_in: stream images must exist), 2^22 (acc_out: they must not), or 2^21 with the multiplier just under
    32000 / 2^21 (travel_in) and exactly that (travel_out).  The site's input is -128 on every feature: tokens of -50.0
    for Q, K, V, fc1 (and LayerNorm1 = -50 by weight 0, bias -50, for fc1 inside the encoder layer); a V of -128 by its biases and mc = 2^-6 for O (a row's probabilities sum to at least 127); for fc2
    the ReLU output is at most 127, by the fc1 biases, so its accumulator reaches 127 * 127 * nnz + top only.
    L: Q = -128 by its biases, K = +127 or -128 per key (one column of Wk, mk = 2^-6), ml at the two sides of
    32000 / (192 * 128 * 128).  E = 64 keeps the fixture's multipliers elsewhere (two of them are refused: the two-rounding
    instantiation), E = 128 takes admitted ones (the single-rounding instantiation wherever the site's own passes)."""
    t0, xf = base(E)
    t = {k: v.copy() for k, v in t0.items()}
    if E == 128:
        for s, mp in passing(E).items():
            set_multiplier(t, s, mp)
    x = np.stack([xf[0], xf[0]]).astype(np.float32)
    x[1, :64], x[1, 64:] = -50.0, 50.0
    if site == "L":
        m_in, m_out = travel_multipliers(L_WORST)
        m = m_in if kind == "travel_in" else m_out
        set_multiplier(t, "L", m)
        set_multiplier(t, "K", f32(2.0 ** -6))
        t["attn0.wq"][:], t["attn0.bq"][:] = 0, -(1 << 20)
        t["attn0.wk"][:], t["attn0.bk"][:] = 0, 0
        t["attn0.wk"][:, 0] = 127
        x[1] = xf[0]
        x[1, 0::2, 0], x[1, 1::2, 0] = 50.0, -50.0
        want = [L_WORST, -192 * 128 * 127]
        return Case(f"E{E}-L-{kind}", E, site, m, kind, (), t, x, want)
    wn, bn = LINEAR[site]
    N, K = t[wn].shape
    travel = kind.startswith("travel")
    nnz = min(K, 128) if travel else K
    total = TRAVEL_SUM if travel else (ACC_BOUND - 1 if kind == "acc_in" else ACC_BOUND)
    top = total - 127 * 128 * nnz
    assert 0 <= top
    r1, r2 = 5, N - 3
    if travel and K > 128:       # the other rows of a wide site stay below the crafted pair's sum
        t[wn][:] = t[wn] // 2
    t[wn][[r1, r2]] = 0
    sg = 1 if site == "fc2" else -1          # the site's input: +127 behind the ReLU, -128 elsewhere
    t[wn][r1, :nnz], t[bn][r1] = 127 * sg, top
    t[wn][r2, :nnz], t[bn][r2] = -127 * sg, -top
    m = multiplier_of(t, site)
    if travel:
        m_in, m_out = travel_multipliers(total)
        assert m_out == f32(125 * 2.0 ** -13)
        m = m_in if kind == "travel_in" else m_out
        set_multiplier(t, site, m)
    reach = total
    if site == "O":
        t["attn0.wv"][:], t["attn0.bv"][:] = 0, -(1 << 20)
        set_multiplier(t, "C", f32(2.0 ** -6))
    if site == "fc1":        # the encoder layer's FFN reads LayerNorm1's output: -50 on every feature, like the frame's tokens
        t["norm1_0.w"][:], t["norm1_0.b"][:] = 0.0, -50.0
    if site == "fc2":
        t["ffn0.w1"][:], t["ffn0.b1"][:] = 0, 1 << 20
        reach = 127 * 127 * nnz + top
    return Case(f"E{E}-{site}-{kind}", E, site, m, kind, (), t, x, [reach, -reach])


def range_inside(case):
    """must this range case get its stream images?"""
    return case.kind.endswith("_in")
