"""Long-sequence attention statistics on the MI355X: ita_mha_long_int8_stats (Engine.attention_stats_long,
attention_received_long, attention_received_map_long) against the numpy definition attention_stats_ref, every comparison
an equality.  Cases and fixtures are long_cases.py's, as in test_gpu_long_taps.py.

Shapes (S, B): (128, 2) one key tile; (256, 2) two; (384, 2) an odd tile count, the ring-slot parity flips between the
sweeps and the column table's slot with it; (1024, 1) eight query tiles adding into one column; (2048, 1) many tiles.  The
crafted frames of long_taps_common give every query of a frame one row of tests/golden/softmax_long_rows.npz, so the
statistics have a closed form (attention_stats_ref.stats_from_row), at 256 and at 8192 keys, with rows the integer softmax
kills among them."""
import functools

import numpy as np
import pytest
import torch

from drone_oa_iree_vit_accelerator_amd import attention_stats_ref as asr
from drone_oa_iree_vit_accelerator_amd import host, params, synth
from heads_common import FIX_HEADS_2L, case as heads_case
from gpu_support import INVALID, UNSUPPORTED, Canaries, captured_replays, cu, refused, to_numpy
from long_cases import FIXTURES, TWO_LAYER, long_case, tap_rows, tokens
import long_taps_common as ltc

pytestmark = pytest.mark.gpu

SHAPES = [(128, 2), (256, 2), (384, 2), (1024, 1)]
STATS = host.LONG_STATS


@functools.lru_cache(maxsize=None)
def _expected(name, S, B):
    """(x, the definition's statistics) of one case: computed once, read-only"""
    case = long_case(name)
    E, t = case.E, case.t
    x = tokens(S + B, B, S, E, t)
    return x, asr.stats(x, t)


def _equal(got, want, msg):
    assert tuple(got) == STATS
    g = to_numpy(got)
    for k in STATS:
        assert g[k].dtype == want[k].dtype and g[k].shape == want[k].shape, (msg, k, g[k].dtype, g[k].shape)
        np.testing.assert_array_equal(g[k], want[k], err_msg=f"{msg} {k}")


def _call(eng, x, st, S=None, B=None):
    host._chk(host.lib().ita_mha_long_int8_stats(eng._h, 0, x.data_ptr() if x is not None else None, B or x.shape[0],
                                                 x.shape[1] if S is None else S,
                                                 host.C.byref(st) if st is not None else None, host._stream_ptr(eng.device)))


def _canaries(B, S):
    return Canaries({k: ((B, S), torch.int8 if k == "row_max" else torch.int32) for k in STATS})


@pytest.mark.parametrize("S,B", SHAPES)
@pytest.mark.parametrize("name", list(FIXTURES))
def test_stats_equal_the_definition(name, S, B):
    case = long_case(name)
    E, t, blob = case.E, case.t, case.blob
    x, want = _expected(name, S, B)
    eng = host.Engine(blob, device=0)
    forms = eng.layer_forms(0)
    assert forms["attn_image"] and (FIXTURES[name] is None or forms["fast"] == FIXTURES[name]), (name, forms)
    xc = cu(x)
    got = eng.attention_stats_long(xc)
    _equal(got, want, f"{name} S={S}")
    assert torch.equal(xc, cu(x)), "x was written to"
    # the taps entry's row maximum and row sum at its rows
    rows = tap_rows(S)
    _, tp = eng._long_taps(xc, rows, 0, ("row_max", "row_sum"))
    for k in ("row_max", "row_sum"):
        assert torch.equal(got[k][:, rows], tp[k]), k
    # the same bytes whatever else is asked for, and twice
    for k in STATS:
        one = eng._long_stats(xc, 0, (k,))
        assert set(one) == {k} and torch.equal(one[k], got[k]), k
    assert torch.equal(eng.attention_received_long(xc), got["col_mass"])
    again = eng.attention_stats_long(xc)
    assert all(torch.equal(again[k], got[k]) for k in STATS)
    # a frame's statistics do not depend on its batch position
    flipped = eng.attention_stats_long(xc.flip(0).contiguous())
    for k in STATS:
        assert torch.equal(flipped[k].flip(0), got[k]), k
    if (name, S) == ("vitlstm_E64_seed1_B2", 384):
        # through the C entry into canary-filled outputs: the column arrays are zeroed by the call, not by the caller
        c = _canaries(B, S)
        _call(eng, xc, host._MhaLongStats(**c.ptrs()))
        _equal(c.views(), want, "canary-filled outputs")
        c.assert_untouched(written=STATS)
    eng.close()


@pytest.mark.parametrize("name", ["vitlstm_E64_seed0_B2", "blocks_E128_seed0_B1"])
def test_many_tiles(name):
    case = long_case(name)
    E, t, blob = case.E, case.t, case.blob
    x, want = _expected(name, 2048, 1)
    eng = host.Engine(blob, device=0)
    _equal(eng.attention_stats_long(cu(x)), want, f"{name} S=2048")
    eng.close()


def _crafted_engine(form):
    eng = host.Engine(ltc.blob(form), device=0)
    forms = eng.layer_forms(0)
    assert forms["attn_image"] and forms["fast"] == (form == "fast"), forms
    return eng


def _equal_row_form(g, b, y, x, S, msg):
    """frame b of the statistics g against the closed form of a frame whose queries all have the logits x, probabilities y"""
    for k, v in asr.stats_from_row(y, S).items():
        assert g[k].dtype == np.int32
        np.testing.assert_array_equal(g[k][b], v, err_msg=f"{msg} {k}")
    np.testing.assert_array_equal(g["row_max"][b], np.full(S, x.max(), np.int8), err_msg=msg)
    np.testing.assert_array_equal(g["row_sum"][b], np.full(S, ltc.row_sums(x), np.int32), err_msg=msg)


@pytest.mark.parametrize("form", ["fast", "exact"])
def test_crafted_rows_256_keys(form):
    """every 256-key row of the fixture as one frame: B = 118, S = 256"""
    d = ltc.fixture()
    assert d["y256"].shape == (118, 256) and int((d["y256"].astype(np.int64).sum(-1) == 0).sum()) == 12
    x = ltc.frames_for(form, d["x256"])
    eng = _crafted_engine(form)
    g = to_numpy(eng.attention_stats_long(cu(x)))
    for b in range(len(x)):
        _equal_row_form(g, b, d["y256"][b], d["x256"][b], 256, f"{form} frame {b}")
    assert int((g["row_mass"][:, 0] == 0).sum()) == 12
    eng.close()


@pytest.mark.parametrize("form", ["fast", "exact"])
def test_crafted_rows_8192_keys(form):
    """the 8192-key rows, one frame per call: three of the five are rows the integer softmax kills"""
    d = ltc.fixture()
    assert [int(v) for v in d["y8192"].astype(np.int64).sum(-1)] == [254, 0, 0, 0, 56]
    x = ltc.frames_for(form, d["x8192"])
    eng = _crafted_engine(form)
    for b in range(len(x)):
        g = to_numpy(eng.attention_stats_long(cu(x[b:b + 1])))
        _equal_row_form(g, 0, d["y8192"][b], d["x8192"][b], 8192, f"{form} row {b}")
        assert g["col_mass"].max() == 8192 * int(d["y8192"][b].max())
    eng.close()


@pytest.mark.parametrize("name", ["vitlstm_E64_seed0_B2", "blocks_E128_seed0_B1"])
def test_random_tokens_8192(name):
    S = 8192
    case = long_case(name)
    E, t, blob = case.E, case.t, case.blob
    eng = host.Engine(blob, device=0)
    xc = cu(tokens(S + 1, 1, S, E, t))
    rows = list(range(3, S, 8))
    assert len(rows) == 1024
    g = to_numpy(eng.attention_stats_long(xc))
    _, tp = eng._long_taps(xc, rows, 0, ("logits", "probs"))
    lg, pr = tp["logits"].cpu().numpy(), tp["probs"].cpu().numpy().astype(np.int64)
    np.testing.assert_array_equal(g["row_max"][:, rows], lg.max(-1))
    np.testing.assert_array_equal(g["row_sum"][:, rows], ltc.row_sums(lg))
    np.testing.assert_array_equal(g["row_mass"][:, rows], pr.sum(-1))
    np.testing.assert_array_equal(g["row_nnz"][:, rows], (pr > 0).sum(-1))
    assert g["row_mass"].astype(np.int64).sum() == g["col_mass"].astype(np.int64).sum()
    assert g["row_nnz"].astype(np.int64).sum() == g["col_nnz"].astype(np.int64).sum()
    assert (g["col_mass"] >= pr.sum(1)).all() and (g["col_nnz"] >= (pr > 0).sum(1)).all()
    assert g["col_mass"].max() > 0
    eng.close()


def test_attention_received_map_long():
    """u8 frames 60 x 90 -> an 8 x 16 and 120 x 180 -> a 16 x 16 token grid, layers 0 and 1 of the two-layer E = 128 blob: the
    composition of tokenize_long, encoder_layer_long and attention_received_long"""
    case = long_case(TWO_LAYER)
    E, nl, t, blob = case.E, case.num_layers, case.t, case.blob
    assert (E, nl) == (128, 2)
    eng = host.Engine(blob, device=0)
    for (H, W), (th, tw) in (((60, 90), (8, 16)), ((120, 180), (16, 16))):
        frames = cu(np.random.RandomState(4).randint(0, 256, size=(2, H, W)).astype(np.uint8))
        for layer in (0, 1):
            got = eng.attention_received_map_long(frames, th, tw, layer=layer)
            assert tuple(got.shape) == (2, th, tw) and got.dtype == torch.int32
            y = eng.tokenize_long(frames, th, tw)
            if layer:
                y = eng.encoder_layer_long(y, 0)
            assert torch.equal(got, eng.attention_received_long(y, layer).reshape(2, th, tw)), (H, W, layer)
            want = asr.stats(y.cpu().numpy(), t, layer)["col_mass"]
            np.testing.assert_array_equal(got.cpu().numpy(), want.reshape(2, th, tw), err_msg=f"{H}x{W} layer {layer}")
    with pytest.raises(ValueError):
        eng.attention_received_map_long(frames, th, tw, layer=2)
    eng.close()


def _refused(eng, status, S=256, seq_len=None, null=False, want=STATS, skew=None):
    """the call must raise with `status` and leave the canary-filled outputs untouched"""
    x = torch.zeros((1, S, eng.E), dtype=torch.float32, device="cuda")
    c = _canaries(1, S)
    st = host._MhaLongStats(**{k: c.ptr(k, 2 if k == skew else 0) for k in want})
    refused(lambda: _call(eng, x, None if null else st, seq_len), c, status)


def test_refusals_before_any_launch_or_memset():
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
    blob = long_case(name).blob
    eng = host.Engine(blob, device=0)
    _refused(eng, UNSUPPORTED, seq_len=200)
    _refused(eng, UNSUPPORTED, seq_len=0)
    _refused(eng, INVALID, null=True)
    _refused(eng, INVALID, want=())
    _refused(eng, INVALID, skew="col_mass")
    x, want = _expected(name, 256, 2)
    _equal(eng.attention_stats_long(cu(x)), want, "after the refusals")
    eng.close()


def test_captured_call_replays():
    """one call captured on one stream: every replay zeroes the column arrays again"""
    name = "vitlstm_E64_seed0_B2"
    blob = long_case(name).blob
    eng = host.Engine(blob, device=0)
    x, want = _expected(name, 256, 2)
    xc = cu(x)
    c = _canaries(2, 256)
    st = host._MhaLongStats(**c.ptrs())
    eager = captured_replays(lambda: eng.attention_stats_long(xc), lambda: _call(eng, xc, st), c, STATS)
    _equal(eager, want, "eager")
    eng.close()
