"""Shared by the long float statistics tests (test_long_f32_stats_cpu.py, test_gpu_long_f32_stats.py): the cases, the
float64 and torch references with the bounds they set, the comparison against attention_stats_f32_ref.stats_from_taps,
and an f32 numpy model of the two sweeps and the addition order of csrc/ita_long_f32_stats_kernel.h.  Everything cached
here is read-only.

Cases: the input kinds of long_f32_common.inputs with the stock blob of long_f32_common.case(E), and 'flat': the plain
input with q_proj times 1 / 8 (float_flat_common.case), where a few dozen keys of every row lie above p_min.

Bounds.  Against the kernels' own probabilities P (stats_from_taps; u = 2^-24, gamma_n = n u / (1 - n u)):
  row_max, row_sum   bit-equal to the taps
  row_nnz, col_nnz   exact
  col_mass           |got - sum_i P| <= gamma_S sum_i P          any fixed-order f32 sum of S non-negative terms
  row_gap            |got - sum_j P (m - s)| <= gamma_(S+2) sum  + one rounding of the difference, one of the product
Against float64 (stats64), per case: 3 e_torch + 4 ulp32(max truth), e_torch the error of torch's CPU f32 evaluation of
softmax(logits).sum(-2) and (softmax (max - logits)).sum(-1) on the same inputs; never GPU output."""
import functools

import numpy as np

from drone_oa_iree_vit_accelerator_amd import attention_stats_f32_ref as asr
import float_flat_common as ffc
import long_f32_common as lc
import long_f32_taps_common as ltc

STATS = ("row_max", "row_sum", "row_gap", "row_nnz", "col_mass", "col_nnz")
P_MIN = 1.0 / 256
ALL_KINDS = ("plain", "ramp", "ramp_rev", "spike_last", "flat")
FLAT_SCALE = 1.0 / 8
# (kind, S, B): all five kinds at S = 256, plain and ramp at the other shapes
CASES = [(k, 256, 2) for k in ALL_KINDS] + [(k, S, B) for S, B in ((128, 3), (384, 2), (1024, 1), (2048, 1)) for k in ("plain", "ramp")]
MUTATIONS = ("max_at_unit", "wave_missing", "lane_missing", "last_tile", "unit_swapped")


def case(kind, E):
    """(float parameters, ITAW0003 blob) of a case; the layer under test is 0"""
    return (ffc.case(E, 0, FLAT_SCALE) if kind == "flat" else lc.case(E))[:2]


def inputs(kind, E, S, B):
    return lc.inputs("plain" if kind == "flat" else kind, E, S, B)


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def refs64(kind, E, S, B):
    """the float64 statistics of a case, and per f32 sum the pair (bound, e_torch)"""
    import torch
    fp, _ = case(kind, E)
    x = inputs(kind, E, S, B)
    t = asr.stats64(x, fp, 0, P_MIN)
    with torch.no_grad():
        F = torch.nn.functional
        w = lambda n: torch.from_numpy(np.asarray(fp[f"attention_blocks.0.{n}"], np.float32).copy())
        xt = torch.from_numpy(x.copy())
        q, k = F.linear(xt, w("q_proj.weight"), w("q_proj.bias")), F.linear(xt, w("k_proj.weight"), w("k_proj.bias"))
        lg = torch.matmul(q, k.transpose(-2, -1))
        sm = torch.softmax(lg, dim=-1)
        r = dict(col_mass=sm.sum(-2).numpy(), row_gap=(sm * (lg.max(-1, keepdim=True).values - lg)).sum(-1).numpy())
    out = dict(t)
    for k in ("col_mass", "row_gap"):
        e = float(np.abs(r[k] - t[k]).max())
        out["bound_" + k] = (3.0 * e + 4.0 * ltc.ulp32(np.abs(t[k]).max()), e)
    return _frozen(out)


def ratios64(got, kind, E, S, B):
    """statistic -> worst error of `got` against float64 as a fraction of the case's bound"""
    t = refs64(kind, E, S, B)
    return {k: float(np.abs(np.asarray(got[k], np.float64) - t[k]).max()) / t["bound_" + k][0] for k in ("col_mass", "row_gap")}


def compare(got, ref, S):
    """got: the six statistics (numpy); ref: stats_from_taps of the same call's taps -> list of what is out of bound"""
    bad = []
    for k in ("row_max", "row_sum"):
        if not np.array_equal(np.asarray(got[k], np.float32).view(np.int32), np.asarray(ref[k], np.float32).view(np.int32)):
            bad.append(f"{k}: not the taps' bits")
    for k in ("row_nnz", "col_nnz"):
        if not np.array_equal(got[k], ref[k]):
            bad.append(f"{k}: {int((np.asarray(got[k]) != ref[k]).sum())} counts differ")
    for k, n in (("col_mass", S), ("row_gap", S + 2)):
        err, lim = np.abs(np.asarray(got[k], np.float64) - ref[k]), asr.gamma(n) * ref[k]
        if not (err <= lim).all():
            i = int(np.argmax(err - lim))
            bad.append(f"{k}: error {err.ravel()[i]:.3e} over gamma_{n} * {ref[k].ravel()[i]:.6e} = {lim.ravel()[i]:.3e}")
    return bad


# ---- the f32 model of the statistics kernel
def logits_f32(kind, E, S, B):
    """the block-summed f32 logits of the kernels (long_f32_taps_common's chains), (B, S, S)"""
    fp, _ = case(kind, E)
    w = ltc._w(fp, 0, np.float32)
    x = inputs(kind, E, S, B)
    return ltc._logits(ltc._project(x, *w["q"], True), ltc._project(x, *w["k"], True), True)


def sweeps(s, p_min=P_MIN, mutation=None):
    """s: (B, S, S) f32 logits -> the six statistics as the two sweeps and the reductions of ita_lf32_stats_kernel and
    ita_lf32_colsum_kernel give them, every addition in the kernel's order.  mutation: one of the wrong kernels the
    tests must tell from the right one:
      'max_at_unit'   p from the running maximum of the unit a key sits in, not the final one
      'wave_missing'  the queries of wave 3 of every tile missing from col_mass and col_nnz
      'lane_missing'  row_gap without the fourth lane share
      'last_tile'     the partial of the last query tile not added
      'unit_swapped'  unit u's column partial stored at unit u ^ 1
      'gt'            p > p_min counted instead of p >= p_min"""
    s = np.asarray(s, np.float32)
    B, S, _ = s.shape
    nu, nqt = S // 64, S // 128
    # sweep 1: the production sweep's m and the four lane shares of l
    m = np.full((B, S), -np.inf, np.float32)
    l = np.zeros((B, S, 4), np.float32)
    m_at = np.empty((B, S, nu), np.float32)
    for u in range(nu):
        su = s[:, :, 64 * u:64 * u + 64]
        mn = np.maximum(m, su.max(-1))
        down = asr.expf(m - mn)
        m = mn
        m_at[:, :, u] = m
        e = asr.expf(su - mn[..., None])
        share = np.zeros((B, S, 4), np.float32)
        for kt in range(4):
            for r in range(4):
                share = share + e[:, :, 16 * kt + r:16 * kt + 16:4]
        l = l * down[..., None] + share
    row_sum = (l[..., 0] + l[..., 1]) + (l[..., 2] + l[..., 3])
    # sweep 2: d = m - s, p = ita_expf(s - m) * (1 / l)
    sub = np.repeat(m_at, 64, axis=-1) if mutation == "max_at_unit" else m[..., None]
    d = sub - s
    p = asr.expf(s - sub) * (np.float32(1.0) / row_sum)[..., None]
    keep = p > np.float32(p_min) if mutation == "gt" else p >= np.float32(p_min)
    pd = p * d
    g = np.zeros((B, S, 4), np.float32)
    for u in range(nu):
        gu = np.zeros((B, S, 4), np.float32)        # the unit's 16 products first, then onto the lane's share
        for kt in range(4):
            for r in range(4):
                gu = gu + pd[:, :, 64 * u + 16 * kt + r:64 * u + 16 * kt + 16:4]
        g = g + gu
    row_gap = (g[..., 0] + g[..., 1]) + (g[..., 2] if mutation == "lane_missing" else g[..., 2] + g[..., 3])
    # columns: 16 query lanes of a wave by rotate-and-add 8, 4, 2, 1; the 8 waves in order; the tiles in order
    v, c = p.reshape(B, nqt, 8, 16, S), keep.reshape(B, nqt, 8, 16, S).astype(np.int32)
    for h in (8, 4, 2, 1):
        v = v[:, :, :, :h] + v[:, :, :, h:]
    v, c = v[:, :, :, 0], c.sum(3)
    if mutation == "wave_missing":
        v, c = v.copy(), c.copy()
        v[:, :, 3], c[:, :, 3] = 0.0, 0
    part = v[:, :, 0]
    for w in range(1, 8):
        part = part + v[:, :, w]
    cpart = c.sum(2)
    if mutation == "unit_swapped":
        swap = lambda a: a.reshape(B, nqt, nu, 64)[:, :, np.arange(nu) ^ 1].reshape(B, nqt, S)
        part, cpart = swap(part), swap(cpart)
    last = nqt - 1 if mutation == "last_tile" else nqt
    col_mass = part[:, 0]
    for t in range(1, last):
        col_mass = col_mass + part[:, t]
    out = dict(row_max=m, row_sum=row_sum, row_gap=row_gap, row_nnz=keep.sum(-1).astype(np.int32), col_mass=col_mass,
               col_nnz=cpart[:, :last].sum(1).astype(np.int32))
    assert all(out[k].dtype == np.float32 for k in ("row_max", "row_sum", "row_gap", "col_mass"))
    return out


@functools.lru_cache(maxsize=None)
def emulated(kind, E, S, B):
    """(logits, statistics) of the f32 model on a case"""
    s = logits_f32(kind, E, S, B)
    s.setflags(write=False)
    return s, _frozen(sweeps(s))


def tie_logits(S=256):
    """one frame whose every row has exactly two equal largest logits and everything else more than 87 below: ita_expf
    gives 1, 1 and S - 2 times e^-87, the row sum rounds to 2.0f and the two probabilities are 0.5f exactly -- a p that
    equals p_min = 0.5.  Row i ties keys i and (i + 77) % S, so every column holds two such values as well."""
    s = np.full((1, S, S), -300.0, np.float32)
    i = np.arange(S)
    s[0, i, i] = 40.0
    s[0, i, (i + 77) % S] = 40.0
    return s
