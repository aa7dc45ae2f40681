"""The exact integer arithmetic the fused requantise and dequantise tests share: m = M 2^-s, the fma's single rounding, the
definition's two roundings, the load-time search's candidates and what it must decide.  The requantise form is derived
in test_requant_fused_cpu.py, the dequantise form (fma32 .. room) in test_dequant_fused_cpu.py.  CPU only."""
from fractions import Fraction

import numpy as np

import requant_common as rc
from conftest import golden_files
from drone_oa_iree_vit_accelerator_amd import host, params

f32 = np.float32
MAGIC128, MAGIC32K, MAGIC0 = 12583040, 12615680, 12582912         # 1.5 * 2^23 + 128, + 32768, + 0 (fc1's ReLU form)
DMAX = 1 << 18


def ms(m):
    """m = M 2^-s, M the 24-bit mantissa"""
    bits = int(f32(m).view(np.uint32))
    ex = bits >> 23
    assert 0 < ex < 255
    return (bits & 0x7FFFFF) | 0x800000, 150 - ex


def cval(C):
    """the float value of the int32 pattern C (exponent field 150: 2^23 + mantissa)"""
    assert 0x4B000000 <= C < 0x4B800000
    return C - 0x4B000000 + (1 << 23)


def amax(m):
    return int(130.0 / float(f32(m))) + 2


def fma_codes(m, C, K, a, logits=False, relu=False):
    """u8 code (or, logits: the clamped signed logit; relu: min(r, 127) saturated at 0) of fma(C + a, m, K) for the int64
    array a, exactly"""
    M, s = ms(m)
    assert float(K) == int(K) and 24 <= s <= 39
    K = int(K)
    N = (cval(C) + a.astype(np.int64)) * M                      # < 2^48
    q, rem, half = N >> s, N & ((1 << s) - 1), 1 << (s - 1)
    r = q + (rem > half) + ((rem == half) & (((q + K) & 1) == 1))
    t = K + r
    assert t.min() >= 1 << 23 and t.max() < 1 << 24               # ulp 1: the rounding above is the fma's
    low = t & 0xFFFF                                              # (t - 2^23 is the mantissa; 2^23 has no low bits)
    if logits:
        return np.clip(low - 32768, -128, 127)
    if relu:
        return np.clip(np.where(low >= 32768, low - 65536, low), 0, 127)
    return np.clip(np.where(low >= 32768, low - 65536, low), 0, 255)


def ref_codes(m, a, logits=False, relu=False):
    """the definition: clamp(rne(fl32(a m))), as the code the u8 saturation yields (+ 128), or the clamped logit, or (relu)
    the code clamped to [0, 127]"""
    r = np.clip(np.rint(a.astype(np.float32) * f32(m)), 0 if relu else -128, 127).astype(np.int64)
    return r if logits or relu else r + 128


def differs(m, C, K, logits=False, relu=False):
    a = np.arange(-amax(m), amax(m) + 1, dtype=np.int64)
    return a[fma_codes(m, C, K, a, logits, relu) != ref_codes(m, a, logits, relu)]


def k_of(m, C, magic=MAGIC128):
    M, s = ms(m)
    return magic - int(round(Fraction(cval(C) * M, 1 << s)))


def candidates(m, dmax=DMAX, n=8):
    """the search's candidates, best first: the n bases within dmax of ACC_BIAS whose C m lies closest to an integer
    (ties: the lower base first), in integer arithmetic"""
    M, s = ms(m)
    d = np.arange(-dmax, dmax + 1, dtype=np.int64)
    fr = ((cval(host.ACC_BIAS) + d) * M) & ((1 << s) - 1)
    dist = np.minimum(fr, (1 << s) - fr)
    return [host.ACC_BIAS + int(d[i]) for i in np.argsort(dist, kind="stable")[:n]]


def proven(m, logits=False, relu=False, dmax=DMAX):
    """what the loader decides for a site: the first candidate the enumeration accepts, or None"""
    if not (0 < float(m) < 1) or 130.0 / float(f32(m)) > 4.0e6:
        return None
    return next((C for C in candidates(m, dmax) if host.fused_check(m, C, logits, relu)[0]), None)


def fixture_multipliers():
    """every attn*.scal[1..6] and ffn*.scal[1..2] of every fixture that holds int8 blocks"""
    out = {}
    for path in golden_files("*.npz"):
        d = params.load_fixture(path)
        for l in range(16):
            if f"attn{l}.q_proj.w_q" in d:
                for j, m in enumerate(params.attention_tensors(d, f"attn{l}.", l)[f"attn{l}.scal"][1:7]):
                    out[f"{path.rsplit('/', 1)[-1][:-4]}.attn{l}.{rc.ATTN_SITES[j]}"] = f32(m)
            if f"ffn{l}.fc1.w_q" in d:
                for j, m in enumerate(params.ffn_tensors(d, f"ffn{l}.", l)[f"ffn{l}.scal"][1:3]):
                    out[f"{path.rsplit('/', 1)[-1][:-4]}.ffn{l}.{rc.FFN_SITES[j]}"] = f32(m)
    return out


# ---- the dequantise form
def fma32(x, m, K):
    """fl32(x * m + K) for an int64 array x of 24-bit integers, a float32 m in (0, 1) and an integer K, as float32"""
    M, s = ms(m)
    assert 24 <= s <= 39 and float(K) == int(K)
    N = x.astype(np.int64) * M + (int(K) << s)
    q, rem, half = N >> s, N & ((1 << s) - 1), 1 << (s - 1)
    t = q + (rem > half) + ((rem == half) & ((q & 1) == 1))
    assert t.min() >= 1 << 23 and t.max() < 1 << 24          # ulp 1: rounding to an integer IS the fma's rounding
    return t.astype(np.float32)


def dequant_codes(m, C, K, a):
    t = fma32(cval(C) + a, m, K)
    r = t - f32(MAGIC0)                                      # exact: both are integers below 2^24
    return np.clip(r, f32(-128.0), f32(127.0)).astype(np.int64)


def dequant_ref_codes(m, a):
    return np.clip(np.rint(a.astype(np.float32) * f32(m)), -128, 127).astype(np.int64)


def dequant_differs(m, C, K):
    a = np.arange(-amax(m), amax(m) + 1, dtype=np.int64)
    return a[dequant_codes(m, C, K, a) != dequant_ref_codes(m, a)]


def in_range(m):
    return 0 < float(m) < 1 and 130.0 / float(f32(m)) <= 4.0e6


def room(w, b):
    """how far the base may move: the worst row of sum |w| * 128 + |b| against 2^22 (prove_fused)"""
    worst = int((np.abs(w.astype(np.int64)).sum(axis=1) * 128 + np.abs(b.astype(np.int64))).max())
    return (1 << 22) - 1 - worst
