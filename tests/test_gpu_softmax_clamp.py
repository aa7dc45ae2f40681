"""Rows whose logits leave the int8 range, through every int8 attention kernel on the MI355X: bit equality with
mha_heads_ref / attention_stats_ref and nothing else.

The stream kernel, the long attention kernel, its taps sibling and the statistics kernel carry their logits UNCLAMPED, as
u = rne(acc ml) + 32768, and fold the reference's clamp into the softmax (m' = clamp(max), shift = min(sub_sat(m', u),
min(m' + 128, 15)); the long kernels requantise the maximum of the raw accumulators).  The frames of softmax_clamp_common
have raw logits of -464 .. 363: a window of int8 width swept across permuted ramps and bands around both ends of the clamp.
tests/test_softmax_clamp_cpu.py counts, per form, among the 768 query rows at S = 128: 194 rows with a raw maximum and more
entries above 127 and entries just below (a), 76 with a clamped maximum in [-127, -114] over entries below -128 (b), 186
wholly below -128 (c), 17 or 18 each with a raw maximum of exactly 127, 128, -128, -129 (d); at S = 256 / 384: 292 / 438
(a), 112 / 168 (b), 72 / 108 (c), and 406 / 609 whose maximum and whose other entries above 127 sit in different key tiles
while every tile has entries outside int8 (e); 80 / 120 dead rows.  Three wrong formulas -- the shift from the unclamped
maximum, no m' + 128 cap, |m' - x| for entries above 127 -- would change probs AND out_q there on 383, 267, 251 rows at
S = 128, on 636, 332, 583 at H = 2, on 512, 136, 512 at S = 256 and on 768, 204, 768 at S = 384, so the routes without taps
see them too.

Each test asserts through Engine.layer_forms that the instantiation it names ran.  The fused-tokenizer image (forward) is
left out: its logits come from pixels and cannot be crafted; it shares the template body with the attention and the
whole-layer image, which are covered."""
import numpy as np
import pytest

from drone_oa_iree_vit_accelerator_amd import host
from gpu_support import UNSUPPORTED, cu, refused_untouched
import long_taps_common as ltc
from requant_common import MHA_TAPS
import softmax_clamp_common as scc

pytestmark = pytest.mark.gpu

FORMS = list(scc.FORMS)
TENSOR, ROW, STATS = host.LONG_TENSOR_TAPS, host.LONG_ROW_TAPS, host.LONG_STATS


def _engine(form, H=1):
    """the crafted blob's engine, on the instantiation the form names (H = 1), or on the block kernels alone (H = 2)"""
    eng = host.Engine(scc.blob(form, H), device=0)
    forms = eng.layer_forms()
    if H == 1:
        assert forms["attn_image"] and forms["layer_image"] and not forms["tok_image"], forms
        assert forms["fast"] == (form == "fast"), forms
    else:
        assert eng.H == 2
        assert forms == dict(fast_sites=0, fast=False, attn_image=False, layer_image=False, tok_image=False)
    return eng


def _equal(got, want, msg):
    g = got.cpu().numpy()
    assert g.dtype == want.dtype and g.shape == want.shape, (msg, g.dtype, g.shape)
    np.testing.assert_array_equal(g, want, err_msg=msg)


@pytest.mark.parametrize("form", FORMS)
def test_block_kernel_taps(form):
    """mha(x, taps=True): ita_mha_kernel<E, 1>, all eight taps and the output; logits are the clamped codes"""
    e = scc.expect(form, "s128")
    eng = _engine(form)
    y, tp = eng.mha(cu(e["x"]), taps=True)
    _equal(tp["logits"], np.clip(e["raw"][:, 0], -128, 127).astype(np.int8), f"{form} logits against the wanted rows")
    for k in MHA_TAPS:
        _equal(tp[k], e["taps"][k], f"{form} tap {k}")
    _equal(y, e["out"], form)
    eng.close()


@pytest.mark.parametrize("form", FORMS)
def test_stream_kernel(form):
    """mha(x), mha_q8(x_q) and encoder_layer(x): ita_softmax_packed16 in the attention image and in the whole-layer image"""
    e = scc.expect(form, "s128")
    eng = _engine(form)
    xc = cu(e["x"])
    _equal(eng.mha(xc), e["out"], f"{form} mha")
    _equal(eng.mha_q8(cu(e["taps"]["x_q"])), e["taps"]["out_q"], f"{form} mha_q8")
    _equal(eng.encoder_layer(xc), e["x2"], f"{form} encoder_layer")
    eng.close()


@pytest.mark.parametrize("form", FORMS)
def test_two_heads(form):
    """the H = 2 blob (head 1's rows are head 0's negated): taps and output of ita_mha_kernel<E, 2>, encoder_layer on the
    block kernels; the int8 entries and the long entry refuse it, as a blob without stream images"""
    e = scc.expect(form, "h2")
    eng = _engine(form, H=2)
    xc = cu(e["x"])
    y, tp = eng.mha(xc, taps=True)
    _equal(tp["logits"], np.clip(e["raw"], -128, 127).astype(np.int8), f"{form} logits against the wanted rows")
    for k in MHA_TAPS:
        _equal(tp[k], e["taps"][k], f"{form} H = 2 tap {k}")
    _equal(y, e["out"], form)
    _equal(eng.mha(xc), e["out"], f"{form} H = 2 mha")
    _equal(eng.encoder_layer(xc), e["x2"], f"{form} H = 2 encoder_layer")
    xq = cu(e["taps"]["x_q"])
    assert refused_untouched(eng, host.lib().ita_mha_q8, xq)
    assert refused_untouched(eng, host.lib().ita_mha_long_q8, xq, 128)
    with pytest.raises(host.ITAError, match=UNSUPPORTED):
        eng.mha_long(xc)
    eng.close()


@pytest.mark.parametrize("S", scc.LONG_S)
@pytest.mark.parametrize("form", FORMS)
def test_long_kernels(form, S):
    """S = 256 (even) and 384 (odd tile count, 120 dead rows), B = 3: mha_long_q8 and mha_long; mha_long_taps with every
    query row asked for, row_max (clamped) and row_sum included; all six statistics"""
    import torch
    e = scc.expect(form, f"long{S}")
    tp = e["taps"]
    eng = _engine(form)
    xc = cu(e["x"])
    _equal(eng.mha_long_q8(cu(tp["x_q"])), tp["out_q"], f"{form} S={S} mha_long_q8")
    y = eng.mha_long(xc)
    _equal(y, e["out"], f"{form} S={S} mha_long")
    rows = list(range(S))
    yt, got = eng.mha_long_taps(xc, rows)
    assert set(got) == set(TENSOR + ROW) and torch.equal(yt, y)
    clamped = np.clip(e["raw"][:, 0], -128, 127)
    want = {k: tp[k] for k in TENSOR + ("logits", "probs")}
    want["row_max"] = clamped.max(-1).astype(np.int8)
    want["row_sum"] = ltc.row_sums(clamped).astype(np.int32)
    _equal(got["logits"], clamped.astype(np.int8), f"{form} S={S} logits against the wanted rows")
    for k in TENSOR + ROW:
        _equal(got[k], want[k], f"{form} S={S} tap {k}")
    st = eng.attention_stats_long(xc)
    assert tuple(st) == STATS
    for k in STATS:
        _equal(st[k], e["stats"][k], f"{form} S={S} statistic {k}")
    np.testing.assert_array_equal(e["stats"]["row_max"], want["row_max"])
    assert int((e["stats"]["row_mass"] == 0).sum()) >= 16            # dead rows, under the definition
    eng.close()


def test_long_batch_position_and_repeat():
    """a frame's result does not depend on its batch position, nor on what ran before: the exact form at S = 384"""
    import torch
    form, S = "exact", 384
    e = scc.expect(form, f"long{S}")
    eng = _engine(form)
    xc = cu(e["x"])
    xf = xc.flip(0).contiguous()
    rows = list(range(0, S, 3))
    y = eng.mha_long(xc)
    _equal(y, e["out"], "first call")
    assert torch.equal(eng.mha_long(xf).flip(0), y) and torch.equal(eng.mha_long(xc), y)
    xq = cu(e["taps"]["x_q"])
    q = eng.mha_long_q8(xq)
    assert torch.equal(eng.mha_long_q8(xq.flip(0).contiguous()).flip(0), q) and torch.equal(eng.mha_long_q8(xq), q)
    _, t1 = eng.mha_long_taps(xc, rows)
    _, tf = eng.mha_long_taps(xf, rows)
    _, t2 = eng.mha_long_taps(xc, rows)
    for k in t1:
        assert torch.equal(tf[k].flip(0), t1[k]) and torch.equal(t2[k], t1[k]), k
    _equal(t1["probs"], e["taps"]["probs"][:, rows], "probs of every third row")
    s1, sf, s2 = eng.attention_stats_long(xc), eng.attention_stats_long(xf), eng.attention_stats_long(xc)
    for k in STATS:
        assert torch.equal(sf[k].flip(0), s1[k]) and torch.equal(s2[k], s1[k]), k
        _equal(s1[k], e["stats"][k], f"statistic {k}")
    eng.close()
