"""Shared by test_softmax_long_cpu.py and test_gpu_long_taps.py: the long-softmax fixture, and blobs crafted so that the
logits of a query row ARE a chosen row of that fixture.

Crafted blob (on requant_common.base(E)'s tensors): wq copies input feature 0 into Q feature 0 and wk input feature 1 into
K feature 0 (weight 2, multiplier 0.5); every other row of wq / wk and both biases are 0.  A token with the code a in
feature 0 and c_j in feature 1 then has logit(q, j) = rne(a c_j ml) against every query, and with a ml = -1 the row is
-c_j: the keys of a frame are one fixture row negated.  Two forms:
    fast   E = 64,  every site's multiplier admitted by the single-rounding proof, a = -128, ml = 2^-7
    exact  E = 128, the fixture's own multipliers (site O is refused), a = -127, ml = float32(1 / 127)
Both ml are below 32000 / (192 * 128 * 128), which the load-time range check of the attention image asks for."""
import functools

import numpy as np

from conftest import golden_files
from drone_oa_iree_vit_accelerator_amd import mha_heads_ref as ref
from drone_oa_iree_vit_accelerator_amd import params
import requant_common as rc

f32 = np.float32
FORMS = {"fast": (64, -128, f32(2.0 ** -7)), "exact": (128, -127, f32(1.0) / f32(127.0))}


@functools.lru_cache(maxsize=None)
def fixture():
    """tests/golden/softmax_long_rows.npz (tools/gen_softmax_long_golden.py); read-only"""
    return params.load_fixture(golden_files("softmax_long_rows.npz")[0])


def row_sums(x):
    """sum of 256 >> (max - x) over the last axis"""
    d = x.astype(np.int64).max(-1, keepdims=True) - x.astype(np.int64)
    return np.where(d > 31, 0, 256 >> np.minimum(d, 31)).sum(-1)


@functools.lru_cache(maxsize=None)
def crafted(form):
    """(E, tensors, query code a) of a form; read-only"""
    E, a, ml = FORMS[form]
    t0, _ = rc.base(E)
    t = {k: v.copy() for k, v in t0.items()}
    if form == "fast":
        for s, mp in rc.passing(E).items():
            rc.set_multiplier(t, s, mp)
    for s in ("Q", "K"):
        rc.set_multiplier(t, s, f32(0.5))
    rc.set_multiplier(t, "L", ml)
    assert float(ml) < 32000.0 / (192 * 128 * 128) and abs(float(f32(a) * ml)) - 1.0 < 1e-6
    for w, b, feat in (("attn0.wq", "attn0.bq", 0), ("attn0.wk", "attn0.bk", 1)):
        t[w][:], t[b][:] = 0, 0
        t[w][0, feat] = 2
    return E, t, a


def blob(form):
    E, t, _ = crafted(form)
    return params.pack_blob(t, E=E, H=1, has_tail=False)


def frames_for(form, logit_rows, seed=3):
    """float frames (len(logit_rows), S, E): frame b's keys produce logit_rows[b] against every query of the frame"""
    E, t, a = crafted(form)
    rows = np.asarray(logit_rows, np.int64)
    assert rows.min() >= -127
    B, S = rows.shape
    codes = np.random.RandomState(seed).randint(-127, 128, size=(B, S, E)).astype(np.int64)
    codes[:, :, 0] = a
    codes[:, :, 1] = -rows
    return rc.codes_to_float(codes, t)


def mha_rows(x, t, rows, l=0):
    """mha_heads_ref.mha's tensors for the query rows `rows` only, from the same functions (a whole S = 8192 frame has
    2^26 logits): (logits, probs, ctx, out_q) of shapes (B, n, S), (B, n, S), (B, n, P), (B, n, E).  test_softmax_long_cpu
    holds it equal to mha itself at S = 256."""
    g = lambda k: t[f"attn{l}.{k}"]
    sc = np.asarray(g("scal"), np.float32)
    x_q = ref.quantize(x, sc[ref.INV_SX])
    Q = ref.linear_q(x_q[:, rows], g("wq"), g("bq"), sc[ref.MQ])
    K, V = ref.linear_q(x_q, g("wk"), g("bk"), sc[ref.MK]), ref.linear_q(x_q, g("wv"), g("bv"), sc[ref.MV])
    logits = ref.requant(Q.astype(np.int32) @ K.astype(np.int32).transpose(0, 2, 1), sc[ref.ML])
    probs = ref.softmax_int(logits)
    ctx = ref.requant(probs.astype(np.int32) @ V.astype(np.int32), sc[ref.MC])
    return logits, probs, ctx, ref.linear_q(ctx, g("wo"), g("bo"), sc[ref.MO])
