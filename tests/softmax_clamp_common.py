"""Shared by test_softmax_clamp_cpu.py and test_gpu_softmax_clamp.py: frames whose RAW logits rne(acc * ml), in front of the
clamp to int8, are chosen integers in about +-600, so that the clamp the stream and long kernels fold into their softmax
(the unclamped 16-bit logit format) decides the result.

long_taps_common.crafted generalised, on the same base tensors and the same two forms (FORMS: fast E = 64, a = -128,
ml = 2^-7; exact E = 128, a = -127, ml = float32(1 / 127)), mq = mk = 0.5.  Per head (H = 1: the whole of P; H = 2: the
same again inside head 1's features):
    wq copies input feature 0 (the code a on every token) into Q features 0 .. N1,
    wk copies input feature 1 (code c1_j) into K features 0 .. N1 - 1 and input feature 2 (code c2_j) into K feature N1,
so rne(acc ml) = -(N1 c1_j + c2_j): with N1 = 4 any integer in +-635.  Behind them the Q features of a second group carry
input feature 3 (code d_q) against K features that are a constant by bk alone (fast: two of 64, bk = 128; exact: one of
127, bk = 254), which adds exactly d_q.  Every other row of wq / wk and both biases are 0; the remaining input features
are random codes, so V, ctx and out_q are real.  Hence
    raw(q, j) = r_j + d_q          (head 1 of the H = 2 blob reads its keys with weight -2:  -r_j + d_q)
and one frame with the base row r and d_q = q - 64 sweeps the clamp window across r in 128 positions.

The classes of query rows the tests count, the kernel's own formula and three wrong ones (stand-ins for a wrong kernel)
are here too, all in numpy on the raw integers."""
import functools

import numpy as np

from drone_oa_iree_vit_accelerator_amd import attention_stats_ref as asr
from drone_oa_iree_vit_accelerator_amd import mha_heads_ref as ref
from drone_oa_iree_vit_accelerator_amd import params
import long_taps_common as ltc
import requant_common as rc

f32 = np.float32
FORMS = ltc.FORMS
N1 = 4
REACH = 127 * (N1 + 1)
LONG_S = (256, 384)
CASES = ("s128", "h2") + tuple(f"long{S}" for S in LONG_S)


@functools.lru_cache(maxsize=None)
def crafted(form, H=1):
    """(E, tensors, query code a) of a form at H heads; read-only"""
    E, a, ml = FORMS[form]
    t0, _ = rc.base(E)
    t = {k: v.copy() for k, v in t0.items()}
    if form == "fast":
        for s, mp in rc.passing(E).items():
            rc.set_multiplier(t, s, mp)
    for s in ("Q", "K"):
        rc.set_multiplier(t, s, f32(0.5))
    rc.set_multiplier(t, "L", ml)
    assert float(ml) < 32000.0 / (192 * 128 * 128)          # the stream images exist (at H = 1)
    for k in ("attn0.wq", "attn0.bq", "attn0.wk", "attn0.bk"):
        t[k][:] = 0
    P = t["attn0.wq"].shape[0]
    assert P % H == 0 and H in (1, 2)
    for h in range(H):
        o, sg = h * (P // H), (1 if h == 0 else -1)
        t["attn0.wq"][o:o + N1 + 1, 0] = 2
        t["attn0.wk"][o:o + N1, 1] = 2 * sg
        t["attn0.wk"][o + N1, 2] = 2 * sg
        g = o + N1 + 1
        n, bk = (2, 128) if form == "fast" else (1, 254)    # K = rne(bk / 2) = 64 twice, or 127 once: the logit gains d_q
        t["attn0.wq"][g:g + n, 3] = 2
        t["attn0.bk"][g:g + n] = bk
    return E, t, a


def blob(form, H=1):
    E, t, _ = crafted(form, H)
    return params.pack_blob(t, E=E, H=H, has_tail=False)


def frames_for(form, rows, d, H=1, seed=3):
    """float frames (B, S, E): raw(b, q, j) = rows[b, j] + d[b, q] on head 0; rows (B, S) integers within +-REACH, d (B, S)"""
    E, t, a = crafted(form, H)
    rows, d = np.asarray(rows, np.int64), np.asarray(d, np.int64)
    assert rows.shape == d.shape and np.abs(rows).max() <= REACH and np.abs(d).max() <= 127
    B, S = rows.shape
    v = -rows
    c1 = np.clip(np.trunc(v / N1).astype(np.int64), -127, 127)
    c2 = v - N1 * c1
    assert np.abs(c2).max() <= 127
    codes = np.random.RandomState(seed).randint(-127, 128, size=(B, S, E)).astype(np.int64)
    codes[:, :, 0], codes[:, :, 1], codes[:, :, 2], codes[:, :, 3] = a, c1, c2, d
    return rc.codes_to_float(codes, t)


def wanted_raw(rows, d, H=1):
    """(B, H, S, S) int64: the raw logits the frames of frames_for must give"""
    rows, d = np.asarray(rows, np.int64), np.asarray(d, np.int64)
    return np.stack([sg * rows[:, None, :] + d[:, :, None] for sg in (1, -1)[:H]], axis=1)


# ---- the wanted rows ---------------------------------------------------------------------------------------------
def _band(rs, lo, hi, n):
    """n integers of [lo, hi] in a seeded order, both ends among them"""
    v = rs.randint(lo, hi + 1, size=n)
    v[:2] = lo, hi
    return rs.permutation(v)


@functools.lru_cache(maxsize=None)
def rows_128():
    """(rows (6, 128), d (6, 128)): a permuted ramp -300 .. 300, the bands -140 .. -121, 120 .. 139 and -400 .. -129 with
    d_q = q - 64; and two bands that end at 127 and at -128 with d_q = q % 8 - 4, so that the raw maximum is exactly 127, 128,
    -128 and -129 on 16 rows each"""
    rs = np.random.RandomState(17)
    S = 128
    rows = np.stack([rs.permutation(np.rint(np.linspace(-300, 300, S)).astype(np.int64)), _band(rs, -140, -121, S),
                     _band(rs, 120, 139, S), _band(rs, -400, -129, S), _band(rs, 112, 127, S), _band(rs, -140, -128, S)])
    q = np.arange(S)
    d = np.stack([q - 64] * 4 + [q % 8 - 4] * 2)
    return rows, d


@functools.lru_cache(maxsize=None)
def rows_long(S):
    """(rows (3, S), d (3, S)), S = 256 or 384.  Frame 0: a permuted ramp -300 .. 300 over all keys.  Frame 1: tile 0 the
    band 120 .. 139, tile 1 the band -140 .. -121 with one key at 200 (the row maximum, away from the other entries above
    127), tile 2 the band -400 .. -129.  Frame 2: nothing above -121 (tiles -140 .. -121, -400 .. -129, -135 .. -129): rows
    that lie wholly below -128 have S equal keys, a row sum of 256 S >= 65 536, and are dead.  d_q sweeps -64 .. 63 in every
    query tile, from another phase in each; on frame 2 it sweeps -16 .. 15, where the maximum is near -128."""
    rs = np.random.RandomState(S)
    nt = S // 128
    assert S in LONG_S
    f1 = [_band(rs, 120, 139, 128), _band(rs, -140, -121, 128), _band(rs, -400, -129, 128)][:nt]
    f1[1][77] = 200
    f2 = [_band(rs, -140, -121, 128), _band(rs, -400, -129, 128), _band(rs, -135, -129, 128)][:nt]
    rows = np.stack([rs.permutation(np.rint(np.linspace(-300, 300, S)).astype(np.int64)), np.concatenate(f1), np.concatenate(f2)])
    q = np.arange(S)
    d = np.stack([(q + 32 * (q // 128)) % 128 - 64] * 2 + [q % 32 - 16])
    return rows, d


def case_rows(case):
    """(rows, d, H) of a case of CASES"""
    if case in ("s128", "h2"):
        return rows_128() + (2 if case == "h2" else 1,)
    return rows_long(int(case[4:])) + (1,)


@functools.lru_cache(maxsize=None)
def expect(form, case):
    """the definition on one case, computed once, read-only: dict of x, t, H, raw (B, H, S, S), out / taps / acc of
    mha_heads_ref.mha, x2 (the encoder layer, S = 128 only) and stats (attention_stats_ref, the long cases only)"""
    from oracle import oracle
    oracle.build()
    rows, d, H = case_rows(case)
    E, t, _ = crafted(form, H)
    x = frames_for(form, rows, d, H)
    out, taps, acc = ref.mha(x, t, H, taps=True)
    e = dict(x=x, t=t, H=H, E=E, raw=wanted_raw(rows, d, H), out=out, taps=taps, acc=acc)
    if x.shape[1] == 128:
        x1 = oracle.add_ln(x, out, t["norm1_0.w"], t["norm1_0.b"])
        e["x2"] = oracle.add_ln(x1, ref.ffn(x1, t)[0], t["norm2_0.w"], t["norm2_0.b"])
    else:
        e["stats"] = asr.stats(x, t)
    return e


# ---- classes of query rows: boolean masks over the leading axes of raw (.., S) ------------------------------------
def class_a(raw):
    """the raw maximum and at least one more entry are above 127, and there are entries 1 .. 8 below 127"""
    return (raw.max(-1) > 127) & ((raw > 127).sum(-1) >= 2) & ((raw >= 119) & (raw <= 126)).any(-1)


def class_b(raw):
    """the clamped maximum is in [-127, -114] and there are raw entries below -128"""
    m = raw.max(-1)
    return (m >= -127) & (m <= -114) & (raw < -128).any(-1)


def class_c(raw):
    """every raw entry is below -128"""
    return raw.max(-1) < -128


def class_d(raw, value):
    """the raw maximum is exactly value (127, 128, -128, -129)"""
    return raw.max(-1) == value


def class_e(raw):
    """the raw maximum lies in a tile of 128 keys other than tile 0; entries above 127 lie in a tile other than the one
    that holds the maximum; every tile holds at least one entry outside the int8 range"""
    S = raw.shape[-1]
    tl = raw.reshape(raw.shape[:-1] + (S // 128, 128))
    holds = (tl == raw.max(-1)[..., None, None]).any(-1)                    # (.., tiles): the tiles that hold the maximum
    above = (tl > 127).any(-1)
    outside = ((tl > 127) | (tl < -128)).any(-1)
    return ~holds[..., 0] & (above & ~holds).any(-1) & outside.all(-1)


# ---- the softmax on raw integers: the definition, the kernels' formula, three wrong formulas -----------------------
def probs_from_shift(shift):
    """mha_heads_ref.softmax_int from its shifts on"""
    shift = shift.astype(np.int64)
    num = np.where(shift > 31, 0, 256 >> np.minimum(shift, 31)).astype(np.int32)
    s = np.maximum(num.sum(-1, keepdims=True), 1)
    inv = np.floor((f32(1.0) / s.astype(np.float32)) * f32(16711680.0)).astype(np.int32)
    return ((num * inv) >> 16).astype(np.uint8)


def shift_definition(raw):
    x = np.clip(raw, -128, 127)
    return x.max(-1, keepdims=True) - x


def shift_kernel(raw):
    """ita_softmax_packed16: m' = clamp(max); shift = min(sub_sat(m', u), min(m' + 128, 15)) on u = raw + 32768"""
    m = np.clip(raw.max(-1, keepdims=True), -128, 127)
    return np.minimum(np.maximum(m - raw, 0), np.minimum(m + 128, 15))


def shift_unclamped_max(raw):
    """wrong: the shift taken from the unclamped maximum"""
    return raw.max(-1, keepdims=True) - np.clip(raw, -128, 127)


def shift_no_cap(raw):
    """wrong: entries below -128 kept at their true distance from the maximum (no m' + 128 cap)"""
    m = np.clip(raw.max(-1, keepdims=True), -128, 127)
    return np.maximum(m - raw, 0)


def shift_abs_above(raw):
    """wrong: entries above 127 given |m' - x| instead of 0"""
    m = np.clip(raw.max(-1, keepdims=True), -128, 127)
    return np.abs(m - np.maximum(raw, -128))


MUTANTS = (shift_unclamped_max, shift_no_cap, shift_abs_above)


def downstream(probs, e):
    """(ctx, out_q) of mha_heads_ref from probabilities (B, H, S, S) on the case e"""
    t = e["t"]
    sc = np.asarray(t["attn0.scal"], np.float32)
    ctx = ref.ctx_from(probs, e["taps"]["V"], e["H"], sc[ref.MC])
    return ctx, ref.linear_q(ctx, t["attn0.wo"], t["attn0.bo"], sc[ref.MO])
