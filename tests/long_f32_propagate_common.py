"""Shared by the long float propagation tests (test_long_f32_propagate_cpu.py, test_gpu_long_f32_propagate.py): the cases,
the weights, the two references with their bounds, and an f32 numpy model of the addition order written down in
csrc/ita_long_f32_prop_kernel.h.  Everything cached here is read-only.

Cases: those of long_f32_stats_common (all five input kinds at S = 256, plain and ramp at the other shapes), E = 64 and 128.

Weights (B, 64, S), different in every frame; row r is of kind ROW_KINDS[r % len(ROW_KINDS)]: all ones, uniform [0, 1),
signed normal, all zero, and one-hot at the queries HOT = 0, 63, 64, 127, 128, S - 1 (a one-hot whose query does not exist
at this S is one-hot at S - 1).  A call with R < 64 rows takes the first R rows, so R = 17 ends on an all-ones row in the
second group and R = 16 on a one-hot.

Bounds.  Against the kernels' own probabilities P (attention_propagate_f32_ref.propagate_from_taps; u = 2^-24):
    |out - sum_i w P| <= gamma_(S+2) sum_i |w| P         any fixed-order f32 sum of S terms, a product, one to spare
one-hot rows bit-equal to P's row, the all-zero row +0.0.  Against float64 from the parameters (propagate64), per case:
3 e_torch + 4 ulp32(max |truth|), e_torch the error of torch's CPU f32 w @ softmax(q k^T) on the same inputs; never GPU
output."""
import functools

import numpy as np

from drone_oa_iree_vit_accelerator_amd import attention_propagate_f32_ref as apr
from drone_oa_iree_vit_accelerator_amd import attention_stats_f32_ref as asr
import long_f32_stats_common as lss
import long_f32_taps_common as ltc

CASES = lss.CASES
R_MAX = 64
RS = (1, 16, 17, 64)
HOT = (0, 63, 64, 127, 128, -1)
ROW_KINDS = ("ones", "uniform", "signed", "zero") + tuple(f"hot{q}" for q in HOT)
MUTATIONS = ("row_shift", "kt_swapped", "unit_missing", "group_alias", "stale_ring", "tile_offset")

case, inputs = lss.case, lss.inputs


def row_kind(r):
    return ROW_KINDS[r % len(ROW_KINDS)]


def hot_query(r, S):
    """the query a one-hot row r points at, or None for the other kinds"""
    k = row_kind(r)
    if not k.startswith("hot"):
        return None
    q = int(k[3:])
    return S - 1 if q < 0 or q >= S else q


@functools.lru_cache(maxsize=None)
def weights(S, B):
    rs = np.random.RandomState(1000 + S + B)
    w = np.zeros((B, R_MAX, S), np.float32)
    for r in range(R_MAX):
        k = row_kind(r)
        if k == "ones":
            w[:, r] = 1.0
        elif k == "uniform":
            w[:, r] = rs.random_sample((B, S)).astype(np.float32)
        elif k == "signed":
            w[:, r] = rs.standard_normal((B, S)).astype(np.float32)
        elif k != "zero":
            w[:, r, hot_query(r, S)] = 1.0
    w.setflags(write=False)
    return w


def rows_of(kind_prefix):
    return [r for r in range(R_MAX) if row_kind(r).startswith(kind_prefix)]


@functools.lru_cache(maxsize=None)
def refs64(kind, E, S, B):
    """(float64 out (B, 64, S), bound, e_torch) of a case"""
    import torch
    fp, _ = case(kind, E)
    x, w = inputs(kind, E, S, B), weights(S, B)
    t = apr.propagate64(x, fp, w, 0, 512)
    with torch.no_grad():
        F = torch.nn.functional
        g = lambda n: torch.from_numpy(np.asarray(fp[f"attention_blocks.0.{n}"], np.float32).copy())
        xt = torch.from_numpy(x.copy())
        q, k = F.linear(xt, g("q_proj.weight"), g("q_proj.bias")), F.linear(xt, g("k_proj.weight"), g("k_proj.bias"))
        r = torch.matmul(torch.from_numpy(w.copy()), torch.softmax(torch.matmul(q, k.transpose(-2, -1)), dim=-1)).numpy()
    e = float(np.abs(r - t).max())
    t.setflags(write=False)
    return t, 3.0 * e + 4.0 * ltc.ulp32(np.abs(t).max()), e


def ratio64(got, kind, E, S, B):
    """worst error of `got` (B, R, S) against float64 as a fraction of the case's bound"""
    t, bound, _ = refs64(kind, E, S, B)
    got = np.asarray(got, np.float64)
    return float(np.abs(got - t[:, :got.shape[1]]).max()) / bound


def compare_taps(got, P, w):
    """got (B, R, S) f32; P (B, S, S) f32 the probabilities of all rows; w (B, R, S) -> (list of what is out of bound,
    worst error / gamma bound over the rows that have one)"""
    got = np.asarray(got, np.float32)
    B, R, S = got.shape
    ref, mass = apr.propagate_from_taps(P, w)
    err, lim = np.abs(got.astype(np.float64) - ref), apr.gamma(S + 2) * mass
    bad = []
    if not (err <= lim).all():
        i = np.unravel_index(int(np.argmax(err - lim)), err.shape)
        bad.append(f"row {i[1]} ({row_kind(i[1])}) frame {i[0]} key {i[2]}: error {err[i]:.3e} over gamma_{S + 2} * {mass[i]:.6e} = {lim[i]:.3e}")
    for r in range(R):
        q = hot_query(r, S)
        if q is not None and not np.array_equal(got[:, r].view(np.int32), np.asarray(P, np.float32)[:, q].view(np.int32)):
            bad.append(f"row {r}: a one-hot row at query {q} does not have the probability row's bits")
        if row_kind(r) == "zero" and not np.array_equal(got[:, r].view(np.int32), np.zeros((B, S), np.int32)):
            bad.append(f"row {r}: the all-zero row is not +0.0 everywhere")
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(lim > 0, err / lim, 0.0)
    return bad, float(ratio.max())


# ---- the f32 model of ita_lf32_prop_kernel
@functools.lru_cache(maxsize=None)
def model_probs(kind, E, S, B):
    """(s, m, inv, p): the block-summed f32 logits (B, S, S) [query, key], the production sweep's row maximum and 1.0f / l,
    and p = ita_expf(s - m) * (1.0f / l) of all rows as the kernel forms it"""
    s, st = lss.emulated(kind, E, S, B)
    m, inv = st["row_max"], (np.float32(1.0) / st["row_sum"]).astype(np.float32)
    p = asr.expf(s - m[..., None]) * inv[..., None]
    for a in (p, inv):
        a.setflags(write=False)
    return s, m, inv, p


def blocked(w, p, mutation=None):
    """w (B, R, S), p (B, S, S) f32 -> out (B, R, S) f32 in the kernel's order: per 64-query unit a block from +0.0f, for kt
    ascending, r4 ascending, slot ascending t = fmaf(w[q], p[q], t) with q = 64 u + 16 kt + 4 slot + r4; then
    acc = acc + t for u ascending.  mutation: see model()"""
    w, p = np.asarray(w, np.float32), np.asarray(p, np.float32)
    B, R, S = w.shape
    nu = S // 64
    if mutation == "group_alias" and R >= 32:
        w = w.copy()
        w[:, 16:32] = w[:, 0:16]
    acc = np.zeros((B, R, S), np.float32)
    for u in range(nu - 1 if mutation == "unit_missing" else nu):
        t = np.zeros((B, R, S), np.float32)
        for kt in range(4):
            wkt = {1: 2, 2: 1}.get(kt, kt) if mutation == "kt_swapped" else kt
            for r4 in range(4):
                for slot in range(4):
                    q, qw = 64 * u + 16 * kt + 4 * slot + r4, 64 * u + 16 * wkt + 4 * slot + r4
                    t = ltc._fma(w[:, :, qw, None], p[:, None, q, :], t)
        acc = acc + t
    if mutation == "tile_offset" and S >= 256:
        acc[:, :, 0:128] = acc[:, :, 128:256]
    assert acc.dtype == np.float32
    return acc


def model(kind, E, S, B, R=R_MAX, mutation=None):
    """the f32 model of the entry on a case, rows 0 .. R - 1.  mutation: one of the wrong kernels the tests must tell
    from the right one:
      'row_shift'     m and 1 / l of the neighbouring query (i + 1, the last query its own)
      'kt_swapped'    the weights of query tiles kt = 1 and 2 of every unit exchanged
      'unit_missing'  the last query unit not added
      'group_alias'   rows 16 .. 31 take the weights of rows 0 .. 15
      'stale_ring'    unit u >= 2 reads unit u - 2's Q (the ring slot was not refilled)
      'tile_offset'   key tile 1 stored at tile 0"""
    s, m, inv, p = model_probs(kind, E, S, B)
    if mutation == "row_shift":
        m2, i2 = np.concatenate([m[:, 1:], m[:, -1:]], 1), np.concatenate([inv[:, 1:], inv[:, -1:]], 1)
        p = asr.expf(s - m2[..., None]) * i2[..., None]
    elif mutation == "stale_ring":
        s2 = np.concatenate([s[:, :128], s[:, :-128]], 1)
        p = asr.expf(s2 - m[..., None]) * inv[..., None]
    with np.errstate(over="ignore", invalid="ignore"):      # a wrong kernel's probabilities may leave f32
        return blocked(weights(S, B)[:, :R], p, mutation)


@functools.lru_cache(maxsize=None)
def modelled(kind, E, S, B):
    out = model(kind, E, S, B)
    out.setflags(write=False)
    return out


def verdict(got, kind, E, S, B):
    """what both bounds say of a full R = 64 result, the probabilities taken from the model: (list of what is out of
    bound, worst error / gamma bound, worst error / float64 bound)"""
    p = model_probs(kind, E, S, B)[3]
    bad, rt = compare_taps(got, p, weights(S, B))
    r64 = ratio64(got, kind, E, S, B)
    if r64 > 1.0:
        bad.append(f"float64: error {r64:.3f} times the bound {refs64(kind, E, S, B)[1]:.3e}")
    return bad, rt, r64
