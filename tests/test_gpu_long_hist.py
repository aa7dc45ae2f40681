"""Long-sequence histograms on the MI355X: ita_mha_long_int8_hist (Engine.attention_histograms_long,
attention_histograms_frames_long) against the numpy definition attention_hist_ref, every comparison an equality.  Fixtures,
shapes and the definition's results are long_hist_common's; test_long_hist_cpu.py holds the inputs to the conditions that
make a kernel which caps the shift histogram at 15, or drops a tile, visibly wrong.

The crafted frames of softmax_clamp_common have raw logits in about +-600, so that logits_out and the two end bins of the
logits histogram are large; the S = 8192 case is held to the blockwise definition."""
import numpy as np
import pytest
import torch

from drone_oa_iree_vit_accelerator_amd import attention_hist_ref as ahr
from drone_oa_iree_vit_accelerator_amd import attention_stats_ref as asr
from drone_oa_iree_vit_accelerator_amd import host, params, synth
from drone_oa_iree_vit_accelerator_amd import mha_heads_ref as ref
from gpu_support import INVALID, UNSUPPORTED, Canaries, captured_replays, cu, refused, to_numpy
from heads_common import FIX_HEADS_2L, case as heads_case
from long_cases import long_case
import long_hist_common as lhc
import softmax_clamp_common as scc

pytestmark = pytest.mark.gpu

NAMES = lhc.NAMES
I64 = ("logits", "shifts", "probs", "logits_out")


def _equal(got, want, msg):
    g = to_numpy(got)
    assert tuple(k for k in g if k in NAMES) == NAMES
    for k in NAMES:
        assert g[k].dtype == want[k].dtype and g[k].shape == want[k].shape, (msg, k, g[k].dtype, g[k].shape)
        np.testing.assert_array_equal(g[k], want[k], err_msg=f"{msg} {k}")


def _call(eng, x, st, S=None, B=None, layer=0):
    host._chk(host.lib().ita_mha_long_int8_hist(eng._h, layer, x.data_ptr() if x is not None else None, B or x.shape[0],
                                                x.shape[1] if S is None else S,
                                                host.C.byref(st) if st is not None else None, host._stream_ptr(eng.device)))


def _canaries(B):
    return Canaries({k: ((B, lhc.WIDTH[k]), torch.int32 if k == "acc_range" else torch.int64) for k in NAMES})


@pytest.mark.parametrize("S,B", lhc.SHAPES)
@pytest.mark.parametrize("name,l", lhc.FIXTURES)
def test_hist_equals_the_definition(name, l, S, B):
    blob = long_case(name).blob
    x, want = lhc.expected(name, l, S, B)
    eng = host.Engine(blob, device=0)
    forms = eng.layer_forms(l)
    assert forms["attn_image"] and forms["fast"] == lhc.FAST[name], (name, forms)
    xc = cu(x)
    got = eng.attention_histograms_long(xc, l)
    _equal(got, want, f"{name} layer {l} S={S}")
    assert torch.equal(xc, cu(x)), "x was written to"
    # the same bytes twice, and whatever the batch position of a frame
    again = eng.attention_histograms_long(xc, l)
    assert all(torch.equal(again[k], got[k]) for k in NAMES)
    flipped = eng.attention_histograms_long(xc.flip(0).contiguous(), l)
    for k in NAMES:
        assert torch.equal(flipped[k].flip(0), got[k]), k
    # each single pointer gives that output alone, through the C entry into canary-filled buffers
    for k in NAMES:
        c = _canaries(B)
        _call(eng, xc, host._MhaLongHist(**c.ptrs((k,))), layer=l)
        torch.cuda.synchronize()
        assert torch.equal(c.views()[k], got[k]), k
        c.assert_untouched(written=(k,))
    eng.close()


def test_stage_histograms():
    name, l, S, B = "vit2l_us_E128_s1_B2", 1, 256, 2
    case = long_case(name)
    t, blob = case.t, case.blob
    x, want = lhc.expected(name, l, S, B)
    eng = host.Engine(blob, device=0)
    got = eng.attention_histograms_long(cu(x), l, stages=True)
    assert tuple(got) == NAMES + host.LONG_HIST_STAGES
    _equal(got, want, "with stages")
    _, tp = ref.mha(x, t, 1, l)
    for k in host.LONG_HIST_STAGES:
        w = np.stack([np.bincount(tp[k][b].astype(np.int64).ravel() + 128, minlength=256) for b in range(B)])
        g = got[k].cpu().numpy()
        assert g.dtype == np.int64 and g.shape == (B, 256), k
        np.testing.assert_array_equal(g, w, err_msg=k)
    eng.close()


@pytest.mark.parametrize("S", lhc.CLAMP_S)
@pytest.mark.parametrize("form", lhc.CLAMP_FORMS)
def test_crafted_clamp_frames(form, S):
    x, want, raw = lhc.clamp_expected(form, S)
    eng = host.Engine(scc.blob(form), device=0)
    forms = eng.layer_forms(0)
    assert forms["attn_image"] and forms["fast"] == (form == "fast"), forms
    g = to_numpy(eng.attention_histograms_long(cu(x)))
    np.testing.assert_array_equal(g["logits_out"], np.stack([(raw < -128).sum((-2, -1)), (raw > 127).sum((-2, -1))], axis=1))
    for k in ("logits", "shifts", "probs", "logits_out"):
        np.testing.assert_array_equal(g[k], want[k], err_msg=k)
    _, _, acc = ref.mha(x, scc.crafted(form)[1], 1, taps=True)
    np.testing.assert_array_equal(g["acc_range"], np.stack([acc["L"].min((1, 2, 3)), acc["L"].max((1, 2, 3))], axis=1))
    eng.close()


def test_frames_entry():
    """u8 frames 60 x 90 -> an 8 x 16 token grid, layers 0 and 1 of the two-layer E = 128 blob: the composition of
    tokenize_long, encoder_layer_long and attention_histograms_long"""
    name = "vit2l_us_E128_s1_B2"
    case = long_case(name)
    nl, t, blob = case.num_layers, case.t, case.blob
    assert nl == 2
    eng = host.Engine(blob, device=0)
    frames = cu(np.random.RandomState(4).randint(0, 256, size=(2, 60, 90)).astype(np.uint8))
    for layer in (0, 1):
        got = eng.attention_histograms_frames_long(frames, 8, 16, layer=layer)
        y = eng.tokenize_long(frames, 8, 16)
        if layer:
            y = eng.encoder_layer_long(y, 0)
        _equal(got, ahr.hist(y.cpu().numpy(), t, layer), f"layer {layer}")
    with pytest.raises(ValueError):
        eng.attention_histograms_frames_long(frames, 8, 16, layer=2)
    eng.close()


def test_captured_call_replays():
    """one call captured on one stream: every replay sets the outputs to zero again"""
    name, l, S, B = "vitlstm_E64_seed0_B2", 0, 256, 2
    blob = long_case(name).blob
    eng = host.Engine(blob, device=0)
    x, want = lhc.expected(name, l, S, B)
    xc = cu(x)
    c = _canaries(B)
    st = host._MhaLongHist(**c.ptrs())
    eager = captured_replays(lambda: eng.attention_histograms_long(xc), lambda: _call(eng, xc, st), c, NAMES)
    _equal(eager, want, "eager")
    eng.close()


def test_8192_keys():
    name, l, S, B = lhc.BIG
    blob = long_case(name).blob
    x, want = lhc.expected(name, l, S, B)
    lhc.conditions(want)
    eng = host.Engine(blob, device=0)
    _equal(eng.attention_histograms_long(cu(x), l), want, f"{name} S={S}")
    eng.close()


def _refused(eng, status, S=256, seq_len=None, null_x=False, null_st=False, want=NAMES, skew=None):
    """the call must raise with `status` and leave the canary-filled outputs untouched"""
    x = torch.zeros((1, S, eng.E), dtype=torch.float32, device="cuda")
    c = _canaries(1)
    st = host._MhaLongHist(**{k: c.ptr(k, 4 if k == skew else 0) for k in want})
    refused(lambda: _call(eng, None if null_x else x, None if null_st else st, S if seq_len is None else seq_len, 1), c, status)


def test_refusals_before_any_launch():
    fpf = synth.float_params(1, E=128, num_layers=2, tail=False)
    ef = host.Engine(params.blob_from_float_params(fpf, 2), device=0)
    _refused(ef, UNSUPPORTED)
    ef.close()
    _, H, E, _, _, _, hblob = heads_case(FIX_HEADS_2L[0])
    assert (H, E) == (4, 128)
    eh = host.Engine(hblob, device=0)
    _refused(eh, UNSUPPORTED)
    eh.close()

    name = "vitlstm_E64_seed0_B2"
    case = long_case(name)
    E, t, blob = case.E, case.t, case.blob
    eng = host.Engine(blob, device=0)
    _refused(eng, UNSUPPORTED, seq_len=200)
    _refused(eng, UNSUPPORTED, seq_len=0)
    _refused(eng, INVALID, null_x=True)
    _refused(eng, INVALID, null_st=True)
    _refused(eng, INVALID, want=())
    for k in I64:
        _refused(eng, INVALID, skew=k)
    x, want = lhc.expected(name, 0, 256, 2)
    _equal(eng.attention_histograms_long(cu(x)), want, "after the refusals")
    st = eng.attention_stats_long(cu(x))
    ws = asr.stats(x, t)
    for k in host.LONG_STATS:
        np.testing.assert_array_equal(st[k].cpu().numpy(), ws[k], err_msg=f"attention_stats_long after the refusals: {k}")
    eng.close()
