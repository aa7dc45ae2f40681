"""Long-sequence int8 attention taps on the MI355X: ita_mha_long_int8_taps (Engine.mha_long_taps, attention_rows_long,
attention_map_long) against the numpy definition mha_heads_ref.mha / softmax_int, every comparison an equality.

The taps kernels are the production kernels' bodies with stores added, so a tap that equals the definition is the value
ita_mha_long_int8 computed with: at S = 256 .. 8192 this is what holds the long kernels' inner tensors, as
ita_mha_int8_taps does at S = 128.

Shapes (S, B): (256, 2) two key tiles; (384, 2) odd tile count, the ring-slot parity flips between the sweeps; (128, 2) one tile, where
every tap must also equal Engine.mha(x, taps=True).  Rows {0, 1, 15, 16, 17, 127, 128, S - 1}: two rows in one wave, waves
with none, the first and the last row, more than one query tile.  Fixtures: E = 64 FAST and exact, E = 128 exact and FAST, and
an ITAW0002 blob (int8 attention, float FFN).

Crafted softmax rows: long_taps_common builds blobs whose logits ARE the rows of tests/golden/softmax_long_rows.npz (row sums at
32 768, around 65 280 where the inverse's high byte runs out, up to 2^21 at 8192 keys); the kernel's logits, row_max,
row_sum and probs must be the fixture's rows and the reference's recorded probabilities, in the FAST and in the exact form."""
import functools

import numpy as np
import pytest

from drone_oa_iree_vit_accelerator_amd import host, params, synth
from drone_oa_iree_vit_accelerator_amd import mha_heads_ref as ref
from heads_common import FIX_HEADS_2L, case as heads_case
from gpu_support import INVALID, UNSUPPORTED, Canaries, cu, refused, to_numpy
from long_cases import FIXTURES, TWO_LAYER, long_case, tap_rows, tokens
import long_taps_common as ltc

pytestmark = pytest.mark.gpu

SHAPES = [(256, 2), (384, 2), (128, 2)]
TENSOR, ROW = host.LONG_TENSOR_TAPS, host.LONG_ROW_TAPS


@functools.lru_cache(maxsize=None)
def _expected(name, S, B):
    """(x, the definition's (out, taps)) of one case: computed once, read-only"""
    c = long_case(name)
    x = tokens(S + B, B, S, c.E, c.t)
    return x, ref.mha(x, c.t, 1, 0)


def _want(tp, rows):
    w = {k: tp[k] for k in TENSOR}
    w["logits"], w["probs"] = tp["logits"][:, rows], tp["probs"][:, rows]
    w["row_max"] = w["logits"].max(-1)
    w["row_sum"] = ltc.row_sums(w["logits"]).astype(np.int32)
    return w


@pytest.mark.parametrize("S,B", SHAPES)
@pytest.mark.parametrize("name", list(FIXTURES))
def test_taps_equal_the_definition(name, S, B):
    import torch
    x, (out, tp) = _expected(name, S, B)
    rows = tap_rows(S)
    eng = host.Engine(long_case(name).blob, device=0)
    forms = eng.layer_forms(0)
    assert forms["attn_image"] and (FIXTURES[name] is None or forms["fast"] == FIXTURES[name]), (name, forms)
    xc = cu(x)
    y, got = eng.mha_long_taps(xc, rows)
    assert set(got) == set(TENSOR + ROW)
    want = _want(tp, rows)
    g = to_numpy(got)
    for k in TENSOR + ROW:
        assert g[k].dtype == want[k].dtype and g[k].shape == want[k].shape, (k, g[k].dtype, g[k].shape)
        np.testing.assert_array_equal(g[k], want[k], err_msg=f"{name} S={S} tap {k}")
    assert torch.equal(y, eng.mha_long(xc)), name
    np.testing.assert_array_equal(y.cpu().numpy(), out, err_msg=name)
    if S == 128:
        y1, t1 = eng.mha(xc, taps=True)
        assert torch.equal(y1, y)
        for k in TENSOR:
            assert torch.equal(t1[k], got[k]), k
        for k in ("logits", "probs"):
            assert torch.equal(t1[k][:, rows], got[k]), k
    # the same bytes whatever else is asked for: no rows, one tap alone, the same call twice
    y0, t0 = eng.mha_long_taps(xc)
    assert set(t0) == set(TENSOR) and torch.equal(y0, y)
    for k in TENSOR:
        assert torch.equal(t0[k], got[k]), k
    for k in TENSOR + ROW:
        y1, t1 = eng._long_taps(xc, rows if k in ROW else (), 0, (k,))
        assert set(t1) == {k} and torch.equal(t1[k], got[k]) and torch.equal(y1, y), k
    y2, t2 = eng.mha_long_taps(xc, rows)
    assert torch.equal(y2, y) and all(torch.equal(t2[k], got[k]) for k in got)
    assert torch.equal(eng.attention_rows_long(xc, rows), got["probs"])
    # a frame's taps do not depend on its batch position
    _, tf = eng.mha_long_taps(xc.flip(0).contiguous(), rows)
    for k in got:
        assert torch.equal(tf[k].flip(0), got[k]), k
    eng.close()


@pytest.mark.parametrize("form", ["fast", "exact"])
def test_crafted_softmax_rows_256_keys(form):
    """every 256-key row of the fixture as one frame's logits: B = number of rows, S = 256"""
    d = ltc.fixture()
    E, t, _ = ltc.crafted(form)
    x = ltc.frames_for(form, d["x256"])
    rows = [0, 17, 128, 255]
    lg, pr, ctx, out_q = ltc.mha_rows(x, t, rows)
    for j in range(len(rows)):                     # on the CPU first: the crafted inputs give the fixture's rows
        np.testing.assert_array_equal(lg[:, j], d["x256"])
        np.testing.assert_array_equal(pr[:, j], d["y256"])
    eng = host.Engine(ltc.blob(form), device=0)
    forms = eng.layer_forms(0)
    assert forms["attn_image"] and forms["fast"] == (form == "fast"), forms
    _, got = eng.mha_long_taps(cu(x), rows)
    g = to_numpy(got)
    for j in range(len(rows)):
        np.testing.assert_array_equal(g["logits"][:, j], d["x256"])
        np.testing.assert_array_equal(g["probs"][:, j], d["y256"])
        np.testing.assert_array_equal(g["row_max"][:, j], d["x256"].max(-1))
        np.testing.assert_array_equal(g["row_sum"][:, j], ltc.row_sums(d["x256"]))
    built = d["sum256"] >= 0
    np.testing.assert_array_equal(g["row_sum"][built, 0], d["sum256"][built])
    np.testing.assert_array_equal(g["ctx"][:, rows], ctx)
    np.testing.assert_array_equal(g["out_q"][:, rows], out_q)
    eng.close()


@pytest.mark.parametrize("form", ["fast", "exact"])
def test_crafted_softmax_rows_8192_keys(form):
    """the 8192-key rows (sums of 65 279, 2^16 + 1, 2^20, 2^21, one random row), one frame per call"""
    d = ltc.fixture()
    E, t, _ = ltc.crafted(form)
    x = ltc.frames_for(form, d["x8192"])
    rows = [0, 129, 4096, 8191]
    lg, pr, ctx, out_q = ltc.mha_rows(x, t, rows)
    for j in range(len(rows)):
        np.testing.assert_array_equal(lg[:, j], d["x8192"])
        np.testing.assert_array_equal(pr[:, j], d["y8192"])
    eng = host.Engine(ltc.blob(form), device=0)
    forms = eng.layer_forms(0)
    assert forms["attn_image"] and forms["fast"] == (form == "fast"), forms
    for b in range(len(x)):
        _, got = eng.mha_long_taps(cu(x[b:b + 1]), rows)
        g = to_numpy(got)
        for j in range(len(rows)):
            np.testing.assert_array_equal(g["logits"][0, j], d["x8192"][b], err_msg=f"row {b}")
            np.testing.assert_array_equal(g["probs"][0, j], d["y8192"][b], err_msg=f"row {b}")
            assert g["row_max"][0, j] == d["x8192"][b].max() and g["row_sum"][0, j] == ltc.row_sums(d["x8192"][b])
        if d["sum8192"][b] >= 0:
            assert g["row_sum"][0, 0] == d["sum8192"][b]
        np.testing.assert_array_equal(g["ctx"][0, rows], ctx[b], err_msg=f"row {b}")
        np.testing.assert_array_equal(g["out_q"][0, rows], out_q[b], err_msg=f"row {b}")
    eng.close()


def _call(eng, x, y, st, S=None):
    host._chk(host.lib().ita_mha_long_int8_taps(eng._h, 0, x.data_ptr(), y.data_ptr(), x.shape[0], S or x.shape[1],
                                               host.C.byref(st) if st is not None else None, host._stream_ptr(eng.device)))


def _refused(eng, status, S=256, rows=(0, 5), n_rows=None, want=TENSOR + ROW, seq_len=None, skew=0):
    """the call must raise with `status` and leave the canary-filled output and taps untouched; skew: bytes added to every
    tap pointer (the buffers are that much larger)"""
    import torch
    B, n = 1, len(rows)
    x = torch.zeros((B, S, eng.E), dtype=torch.float32, device="cuda")
    shapes = dict(x_q=(B, S, eng.E), out_q=(B, S, eng.E), Q=(B, S, eng.P), K=(B, S, eng.P), V=(B, S, eng.P), ctx=(B, S, eng.P),
                  logits=(B, max(n, 1), S), probs=(B, max(n, 1), S), row_max=(B, max(n, 1)), row_sum=(B, max(n, 1)))
    dt = dict(probs=torch.uint8, row_sum=torch.int32)
    c = Canaries({"y": (x.shape, torch.float32), **{k: (shapes[k], dt.get(k, torch.int8)) for k in want}})
    st = host._MhaLongTaps(**{k: c.ptr(k, skew) for k in want})
    arr = (host.C.c_int * max(n, 1))(*rows)
    st.rows, st.n_rows = (arr if n else None), (n if n_rows is None else n_rows)
    refused(lambda: _call(eng, x, c.views()["y"], st, seq_len), c, status)


def test_refusals_before_any_launch():
    import torch
    fpf = synth.float_params(1, E=128, num_layers=2, tail=False)
    ef = host.Engine(params.blob_from_float_params(fpf, 2), device=0)
    _refused(ef, UNSUPPORTED)
    assert "no row probabilities" in host.lib().ita_error_string().decode()
    ef.close()
    _, H, E, _, _, _, hblob = heads_case(FIX_HEADS_2L[0])
    assert (H, E) == (4, 128)
    eh = host.Engine(hblob, device=0)
    _refused(eh, UNSUPPORTED)
    eh.close()

    name = "vitlstm_E64_seed0_B2"
    eng = host.Engine(long_case(name).blob, device=0)
    _refused(eng, UNSUPPORTED, S=256, seq_len=200)                       # not a multiple of 128
    _refused(eng, INVALID, rows=(0, 5), n_rows=-1)
    _refused(eng, INVALID, rows=(0, 5), n_rows=1025)
    _refused(eng, INVALID, rows=(), n_rows=2)                            # n_rows > 0 without rows
    _refused(eng, INVALID, rows=(5, 5))                                  # not strictly increasing
    _refused(eng, INVALID, rows=(7, 3))
    _refused(eng, INVALID, rows=(0, 256))                                # out of range
    _refused(eng, INVALID, rows=(-1, 3))
    for k in ROW:                                                        # a row-indexed pointer with n_rows == 0
        _refused(eng, INVALID, rows=(), want=(k,))
    _refused(eng, INVALID, rows=(), want=("x_q",), skew=4)               # x_q must be 16-byte aligned
    _refused(eng, INVALID, rows=(0, 5), want=("probs",), skew=1)         # probs 4-byte aligned
    # the most rows there may be are served, and the handle still computes mha_long
    x, (out, tp) = _expected(name, 256, 2)
    xc = cu(np.concatenate([x, x, x, x], axis=1))                        # S = 1024
    many = list(range(1024))
    probs = eng.attention_rows_long(xc, many)
    assert tuple(probs.shape) == (2, 1024, 1024)
    np.testing.assert_array_equal(eng.mha_long(cu(x)).cpu().numpy(), out)
    y, got = eng.mha_long_taps(cu(x), [3])
    np.testing.assert_array_equal(got["probs"].cpu().numpy(), tp["probs"][:, [3]])
    # taps == NULL behaves as all-null taps
    y0 = torch.empty_like(y)
    _call(eng, cu(x), y0, None)
    assert torch.equal(y0, y)
    eng.close()


def test_refused_inside_a_stream_capture():
    import torch
    name = "vitlstm_E64_seed0_B2"
    eng = host.Engine(long_case(name).blob, device=0)
    x, (out, _) = _expected(name, 256, 2)
    xc = cu(x)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eng.mha_long(xc)                            # warm-up outside the capture: the workspace exists
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    y = torch.full_like(xc, 12345.0)
    yg = torch.empty_like(xc)
    g = torch.cuda.CUDAGraph()
    message = None
    with torch.cuda.graph(g):
        host._chk(host.lib().ita_mha_long_int8(eng._h, 0, xc.data_ptr(), yg.data_ptr(), 2, 256, host._stream_ptr(eng.device)))
        try:
            _call(eng, xc, y, host._MhaLongTaps())
        except host.ITAError as e:
            message = str(e)
    assert message is not None and INVALID in message and "capture" in message, message
    g.replay()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(yg.cpu().numpy(), out)
    assert bool((y == 12345.0).all())
    del g
    eng.close()


def test_attention_map_long():
    """20 x 30 u8 frames -> an 8 x 32 token grid, two queries in descending order, layers 0 and 1 of the two-layer E = 128
    blob: the composition of tokenize_long, encoder_layer_long and the definition's probabilities"""
    c = long_case(TWO_LAYER)
    assert (c.E, c.num_layers) == (128, 2)
    eng = host.Engine(c.blob, device=0)
    frames = cu(np.random.RandomState(4).randint(0, 256, size=(2, 20, 30)).astype(np.uint8))
    th, tw, queries = 8, 32, [(5, 17), (2, 3)]
    toks = [ty * tw + tx for ty, tx in queries]
    for layer in (0, 1):
        got = eng.attention_map_long(frames, th, tw, queries, layer=layer)
        assert tuple(got.shape) == (2, 2, th, tw) and got.dtype.is_floating_point is False
        y = eng.tokenize_long(frames, th, tw)
        for l in range(layer):
            y = eng.encoder_layer_long(y, l)
        _, tp = ref.mha(y.cpu().numpy(), c.t, 1, layer)
        np.testing.assert_array_equal(got.cpu().numpy(), tp["probs"][:, toks].reshape(2, 2, th, tw), err_msg=f"layer {layer}")
        assert len(np.unique(got.cpu().numpy())) > 2
    with pytest.raises(ValueError):
        eng.attention_map_long(frames, th, tw, [(1, 1), (1, 1)])
    with pytest.raises(ValueError):
        eng.attention_map_long(frames, th, tw, [(8, 0)])
    eng.close()
