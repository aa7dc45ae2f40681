"""Per-head long-sequence histograms on the MI355X: ita_mha_long_heads_int8_hist (csrc/ita_long_heads_hist_kernel.h), every
array equal to attention_hist_heads_ref.hist_heads (integers: assert_array_equal).  Weights and inputs are
test_gpu_long_heads_stats.py's: E = 64 selects the FAST instantiations, E = 128 the exact ones; long_f32, seed 5."""
import functools

import numpy as np
import pytest
import torch

from drone_oa_iree_vit_accelerator_amd import host, mha_heads_ref, params, synth
from drone_oa_iree_vit_accelerator_amd.attention_hist_heads_ref import NAMES, hist_heads, hist_heads_from_classes
from gpu_support import INVALID, UNSUPPORTED, Canaries, captured_replays, cu, engine_pool, refused, to_numpy
from heads_common import FIX_HEADS, FIX_HEADS_2L, case, heads_of
from long_cases import long_f32

pytestmark = pytest.mark.gpu

SEED = 5


def weights(E):
    d, _, _, nl, t, fp, _ = case([p for p in FIX_HEADS if heads_of(p) == 3][0] if E == 64 else FIX_HEADS_2L[0])
    return d, nl, t, fp


@functools.lru_cache(maxsize=None)
def blob(E, H):
    d, nl, _, fp = weights(E)
    return params.blob_from_record(d, fp, E=E, num_layers=nl, H=H)


@pytest.fixture(scope="module")
def engines():
    yield from engine_pool(blob)


@functools.lru_cache(maxsize=None)
def reference(E, H, S, B=2, scale=1.0):
    """(x, hist_heads of it) for the module's inputs, times `scale`; read-only"""
    t = weights(E)[2]
    x = long_f32(SEED, B, S, E, t) * np.float32(scale)
    return x, hist_heads(x, t, H)


def equal(got, want):
    got = to_numpy(got)
    assert tuple(k for k in got if k in NAMES) == NAMES
    for k in NAMES:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


def canaries(B, H):
    return Canaries({k: ((B, H, 2 if k in ("logits_out", "acc_range") else 256), torch.int32 if k == "acc_range" else torch.int64) for k in NAMES})


def call(eng, xc, st, S=None):
    host._chk(host.lib().ita_mha_long_heads_int8_hist(eng._h, 0, xc.data_ptr(), xc.shape[0], xc.shape[1] if S is None else S,
                                                      host.C.byref(st), host._stream_ptr(eng.device)))


@pytest.mark.parametrize("S", [128, 256, 384])
@pytest.mark.parametrize("H", [2, 3, 4, 6])
@pytest.mark.parametrize("E", [64, 128])
def test_definition(engines, E, H, S):
    """one, two, three key tiles: the ring wraps between the passes at both parities; times 3.0 every head clamps on both sides"""
    x, want = reference(E, H, S)
    assert want["logits_out"].sum() <= (0 if E == 64 else 2), want["logits_out"]
    assert (want["shifts"][..., 16:].sum(-1) > 0).all() and (want["logits"][:, 0] != want["logits"][:, 1]).any(), "no large shifts, or heads alike"
    equal(engines(E, H).attention_histograms_long_heads(cu(x)), want)
    x3, want3 = reference(E, H, S, scale=3.0)
    assert (want3["logits_out"] > 0).all(), want3["logits_out"]
    if S == 256:
        assert (want3["logits"] > 0).all() and want3["logits_out"].min() >= 94, want3["logits_out"].min()
    equal(engines(E, H).attention_histograms_long_heads(cu(x3)), want3)


@pytest.mark.parametrize("E,H", [(64, 3), (128, 4)])
def test_flat_keys(engines, E, H):
    """test_gpu_long_heads_stats.py's S = 2048 flat-key frame: 1920 x 1920 entries of a head fall into one bin of each histogram"""
    t = weights(E)[2]
    x = long_f32(SEED, 1, 2048, E, t).copy()
    x[:, 128:] = x[:, 600]
    want = hist_heads(x, t, H)
    assert all((want[k].max(-1) >= 1920 * 1920).all() for k in ("logits", "shifts", "probs"))
    equal(engines(E, H).attention_histograms_long_heads(cu(x)), want)


@pytest.mark.parametrize("E,H", [(64, 6), (128, 2)])
def test_65536_keys(engines, E, H):
    """512 distinct token rows, one at half of the positions, the rest sharing the other half evenly: the hottest bin holds
    2^30 entries (a workgroup's share 2^22, a wave's 2^19), every histogram sums to 2^32; against the 512 x 512 class form"""
    S, t = 65536, weights(E)[2]
    reps = long_f32(SEED, 1, 512, E, t)[0]
    counts = np.r_[S // 2, np.full(511, 64) + (np.arange(511) < S // 2 - 511 * 64)]
    assert counts.sum() == S
    x = reps[np.random.RandomState(SEED).permutation(np.repeat(np.arange(512), counts))][None]
    want = hist_heads_from_classes(reps, counts, t, H)
    for k in ("logits", "shifts", "probs"):
        assert (want[k].sum(-1) == 1 << 32).all() and (want[k].max(-1) >= 1 << 30).all(), k
    equal(engines(E, H).attention_histograms_long_heads(cu(x)), want)


def test_single_pointers_repeat_and_batch(engines):
    """each pointer alone gives that output and touches nothing else; a second call the same bytes; frame b is the B = 1 call"""
    E, H, S = 128, 6, 384
    eng, (x, want) = engines(E, H), reference(E, H, S, 3)
    xc = cu(x)
    first = eng.attention_histograms_long_heads(xc)
    equal(eng.attention_histograms_long_heads(xc), to_numpy(first))
    equal(first, want)
    for k in NAMES:
        c = canaries(3, H)
        call(eng, xc, host._MhaLongHist(**c.ptrs((k,))))
        torch.cuda.synchronize()
        assert torch.equal(c.views()[k], first[k]), k
        c.assert_untouched(written=(k,))
    for b in range(3):
        equal(eng.attention_histograms_long_heads(cu(x[b:b + 1])), {k: v[b:b + 1] for k, v in want.items()})


def test_one_head_and_refusals(engines):
    """H = 1 forwards; S = 200, a float blob, all-NULL and a skewed s64 pointer are refused untouched; the one-head entry refuses H > 1"""
    E, S = 64, 256
    e1, e3 = engines(E, 1), engines(E, 3)
    x, want = reference(E, 1, S)
    xc = cu(x)
    got = e1.attention_histograms_long_heads(xc)
    equal(got, want)
    equal({k: v[:, None] for k, v in e1.attention_histograms_long(xc).items()}, to_numpy(got))
    c = canaries(2, 3)
    refused(lambda: call(e3, xc, host._MhaLongHist(**c.ptrs()), S=200), c, UNSUPPORTED)
    refused(lambda: call(e3, xc, host._MhaLongHist()), c, INVALID)
    refused(lambda: call(e3, xc, host._MhaLongHist(**{k: c.ptr(k, 4 if k == "shifts" else 0) for k in NAMES})), c, INVALID)
    ef = host.Engine(params.blob_from_float_params(synth.float_params(1, E=64, num_layers=1, tail=True), 1), device=0)
    refused(lambda: call(ef, xc, host._MhaLongHist(**c.ptrs())), c, UNSUPPORTED)
    ef.close()
    with pytest.raises(host.ITAError, match=UNSUPPORTED):
        e3.attention_histograms_long(xc)
    equal(e3.attention_histograms_long_heads(xc), reference(E, 3, S)[1])


def test_captured_call_replays(engines):
    """one call captured on one stream: every replay sets the outputs to zero again"""
    E, H, S = 64, 4, 256
    eng, (x, want), c = engines(E, H), reference(E, H, S), canaries(2, H)
    xc, st = cu(x), host._MhaLongHist(**c.ptrs())
    equal(captured_replays(lambda: eng.attention_histograms_long_heads(xc), lambda: call(eng, xc, st), c, NAMES), want)


def test_stage_histograms(engines):
    E, H, S = 128, 3, 256
    x, want = reference(E, H, S)
    got = engines(E, H).attention_histograms_long_heads(cu(x), stages=True)
    assert tuple(got) == NAMES + host.LONG_HIST_STAGES
    equal(got, want)
    _, tp = mha_heads_ref.mha(x, weights(E)[2], H)
    count = lambda a: np.stack([np.bincount(r.astype(np.int64).ravel() + 128, minlength=256) for r in a])
    for k in host.LONG_HIST_STAGES:
        w = count(tp[k]) if k in ("x_q", "out_q") else count(mha_heads_ref.split_heads(tp[k], H).reshape(2 * H, -1)).reshape(2, H, 256)
        np.testing.assert_array_equal(got[k].cpu().numpy(), w, err_msg=k)


def test_frames_entry(engines):
    """u8 frames 60 x 90 -> 8 x 16 tokens, layers 0 and 1: tokenize_long, encoder_layer_long_heads and hist_heads composed"""
    E, H = 128, 4
    eng, t = engines(E, H), weights(E)[2]
    frames = cu(np.random.RandomState(4).randint(0, 256, size=(2, 60, 90)).astype(np.uint8))
    for layer in (0, 1):
        got = eng.attention_histograms_frames_long_heads(frames, 8, 16, layer=layer)
        y = eng.tokenize_long(frames, 8, 16)
        if layer:
            y = eng.encoder_layer_long_heads(y, 0)
        equal(got, hist_heads(y.cpu().numpy(), t, H, layer))
    with pytest.raises(ValueError):
        eng.attention_histograms_frames_long_heads(frames, 8, 16, layer=2)
