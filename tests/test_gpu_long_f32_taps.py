"""Long float attention taps on the MI355X: ita_mha_long_f32_taps (Engine.mha_long_f32_taps, attention_rows_long_f32,
attention_map_long_f32) on ITAW0003 blobs.

The taps kernels are the production kernels' bodies with stores added, so y must equal mha_long_f32 bit for bit and a tap
is the value the launches computed with.  The taps are f32, so they are held to float64 by the bounds of
tests/long_f32_taps_common.py (torch's own f32 error on the same rows sets them, never GPU output); what IS exact is
checked as an equality: row_max == logits.max(-1), and probs == ita_expf(logits - row_max) * (1.0f / row_sum) from the
returned taps, through the oracle's ita_oracle_expf.

Shapes (S, B) = lc.SHAPES: 128 is one query tile and two units, 256 wraps the K ring and has a second query tile, 384
has an odd tile count, 1024 has 16 units.  E = 64 with layer 0, E = 128 with layers 0 and 1.  Rows: long_f32_taps_common.rows_for
(the tile and sequence boundaries plus the four least peaked rows of frame 0)."""
import numpy as np
import pytest

from drone_oa_iree_vit_accelerator_amd import host
from gpu_support import INVALID, UNSUPPORTED, Canaries, cu, engine_pool, refused, to_numpy
from long_cases import long_case
import long_f32_common as lc
import long_f32_taps_common as ltc

pytestmark = pytest.mark.gpu

MODELS = [(64, 0), (128, 0), (128, 1)]
KINDS = ("plain", "ramp", "spike_first")
TENSOR, ROW = host.LONG_F32_TENSOR_TAPS, host.LONG_ROW_TAPS
SENTINEL, PAD = 12345.0, 64       # PAD: bytes behind every tap buffer


@pytest.fixture(scope="module")
def engines():
    yield from engine_pool(lambda E: lc.case(E)[1])


def _probs_from_taps(g):
    """the definition of the probs tap, from the returned logits, row_max and row_sum, each step rounded to f32"""
    inv = (np.float32(1.0) / g["row_sum"]).astype(np.float32)
    return (ltc.expf((g["logits"] - g["row_max"][..., None]).astype(np.float32)) * inv[..., None]).astype(np.float32)


def _check_bounds(g, kind, E, S, B, layer, rows):
    bnd, err = ltc.bounds(kind, E, S, B, layer, rows), ltc.errors(g, kind, E, S, B, layer, rows)
    for k in err:
        print(f"{kind} E={E} layer {layer} S={S} B={B} {k}: |gpu - float64| = {err[k]:.3e}, e_torch {bnd[k][1]:.3e}, "
              f"bound {bnd[k][0]:.3e}, err / bound {err[k] / bnd[k][0]:.2f}")
    for k in err:
        assert np.isfinite(g[k]).all() and err[k] <= bnd[k][0], (k, err[k], bnd[k])


def _call(eng, x, y, st, S=None, layer=0):
    host._chk(host.lib().ita_mha_long_f32_taps(eng._h, layer, x.data_ptr(), y.data_ptr(), x.shape[0], S or x.shape[1],
                                              host.C.byref(st) if st is not None else None, host._stream_ptr(eng.device)))


@pytest.mark.parametrize("S,B", lc.SHAPES)
@pytest.mark.parametrize("E,layer", MODELS)
@pytest.mark.parametrize("kind", KINDS)
def test_taps_against_float64(engines, kind, E, layer, S, B):
    import torch
    eng = engines(E)
    x = cu(lc.inputs(kind, E, S, B))
    rows = ltc.rows_for(kind, E, S, B, layer)
    y, got = eng.mha_long_f32_taps(x, rows, layer)
    assert set(got) == set(TENSOR + ROW)
    want_y = eng.mha_long_f32(x, layer)
    assert torch.equal(y, want_y)
    g = to_numpy(got)
    for k in TENSOR:
        assert g[k].shape == (B, S, eng.P) and g[k].dtype == np.float32, k
    assert g["logits"].shape == g["probs"].shape == (B, len(rows), S) and g["row_max"].shape == g["row_sum"].shape == (B, len(rows))
    _check_bounds(g, kind, E, S, B, layer, rows)
    np.testing.assert_array_equal(g["row_max"], g["logits"].max(-1))
    np.testing.assert_array_equal(g["probs"], _probs_from_taps(g))
    # y whatever is asked for: rows only, a NULL struct
    y1, t1 = eng._long_f32_taps(x, rows, layer, ROW)
    assert torch.equal(y1, want_y) and all(torch.equal(t1[k], got[k]) for k in ROW)
    y0 = torch.full_like(x, SENTINEL)
    _call(eng, x, y0, None, layer=layer)
    assert torch.equal(y0, want_y)
    # each tap alone is the same tap asked for with all the others; two runs are bit-identical
    for k in TENSOR + ROW:
        y1, t1 = eng._long_f32_taps(x, rows if k in ROW else (), layer, (k,))
        assert set(t1) == {k} and torch.equal(t1[k], got[k]) and torch.equal(y1, want_y), k
    y2, t2 = eng.mha_long_f32_taps(x, rows, layer)
    assert torch.equal(y2, y) and all(torch.equal(t2[k], got[k]) for k in got)
    assert torch.equal(eng.attention_rows_long_f32(x, rows, layer), got["probs"])


@pytest.mark.parametrize("E,layer", MODELS)
def test_row_counts(engines, E, layer):
    """no rows with the four tensors, one row, all 128 rows of one tile"""
    import torch
    eng, kind, (S, B) = engines(E), "plain", lc.SHAPES[0]
    x = cu(lc.inputs(kind, E, S, B))
    want_y = eng.mha_long_f32(x, layer)
    _, full = eng.mha_long_f32_taps(x, range(S), layer)
    g = to_numpy(full)
    _check_bounds(g, kind, E, S, B, layer, range(S))
    np.testing.assert_array_equal(g["row_max"], g["logits"].max(-1))
    np.testing.assert_array_equal(g["probs"], _probs_from_taps(g))
    y0, t0 = eng.mha_long_f32_taps(x, (), layer)
    assert set(t0) == set(TENSOR) and torch.equal(y0, want_y) and all(torch.equal(t0[k], full[k]) for k in TENSOR)
    for r in (0, 77, S - 1):
        y1, t1 = eng.mha_long_f32_taps(x, [r], layer)
        assert torch.equal(y1, want_y)
        for k in ROW:
            assert torch.equal(t1[k], full[k][:, r:r + 1]), (k, r)


def test_the_most_rows(engines):
    """1024 rows at S = 1024, B = 1: every query of eight tiles, the most rows there may be"""
    import torch
    E, kind, layer, (S, B) = 64, "plain", 0, lc.SHAPES[3]
    assert (S, B) == (1024, 1)
    eng = engines(E)
    x = cu(lc.inputs(kind, E, S, B))
    y, got = eng._long_f32_taps(x, range(S), layer, ROW)
    assert torch.equal(y, eng.mha_long_f32(x, layer))
    g = to_numpy(got)
    _check_bounds(g, kind, E, S, B, layer, range(S))
    np.testing.assert_array_equal(g["row_max"], g["logits"].max(-1))
    np.testing.assert_array_equal(g["probs"], _probs_from_taps(g))
    rows = ltc.rows_for(kind, E, S, B, layer)
    _, few = eng.mha_long_f32_taps(x, rows, layer)
    for k in ROW:
        assert torch.equal(few[k], got[k][:, list(rows)]), k


def _canaries(eng, B, S, n, want, y=False):
    """canary-filled f32 buffers of the taps in `want`, PAD bytes behind each; y: one for the (B, S, E) output as well"""
    import torch
    shape = dict(Q=(B, S, eng.P), K=(B, S, eng.P), V=(B, S, eng.P), ctx=(B, S, eng.P), logits=(B, max(n, 1), S),
                 probs=(B, max(n, 1), S), row_max=(B, max(n, 1)), row_sum=(B, max(n, 1)), y=(B, S, eng.E))
    return Canaries({k: (shape[k], torch.float32) for k in tuple(want) + (("y",) if y else ())}, pad=PAD)


@pytest.mark.parametrize("E,layer", MODELS)
def test_canaries_and_frame_independence(engines, E, layer):
    import torch
    eng, kind, (S, B) = engines(E), "ramp", lc.SHAPES[1]
    assert B == 2
    x = cu(lc.inputs(kind, E, S, B))
    rows = ltc.rows_for(kind, E, S, B, layer)
    y, got = eng.mha_long_f32_taps(x, rows, layer)
    c = _canaries(eng, B, S, len(rows), TENSOR + ROW)
    st = host._MhaLongF32Taps(**c.ptrs())
    arr = (host.C.c_int * len(rows))(*rows)
    st.rows, st.n_rows = arr, len(rows)
    y1 = torch.empty_like(x)
    _call(eng, x, y1, st, layer=layer)
    torch.cuda.synchronize()
    assert torch.equal(y1, y)
    c.assert_untouched(written=TENSOR + ROW)
    for k, v in c.views().items():
        assert torch.equal(v.reshape(got[k].shape), got[k]), k
    # frame 1 of the batch equals the same frame run alone
    ya, ta = eng.mha_long_f32_taps(x[1:2].contiguous(), rows, layer)
    assert torch.equal(ya, y[1:2])
    for k in got:
        assert torch.equal(ta[k], got[k][1:2]), k


@pytest.mark.parametrize("E,layer", [(64, 0), (128, 1)])
def test_attention_map_long_f32(engines, E, layer):
    """2 frames of 97 x 131 -> an 8 x 16 token grid, queries out of order: tokenize_long, the layers below, the rows"""
    import torch
    eng = engines(E)
    frames = cu(np.random.RandomState(4).randint(0, 256, size=(2, 97, 131)).astype(np.uint8))
    th, tw, queries = 8, 16, [(5, 11), (0, 3), (7, 15)]
    toks = [ty * tw + tx for ty, tx in queries]
    got = eng.attention_map_long_f32(frames, th, tw, queries, layer=layer)
    assert tuple(got.shape) == (2, 3, th, tw) and got.dtype == torch.float32
    y = eng.tokenize_long(frames, th, tw)
    for l in range(layer):
        y = eng.encoder_layer_long_f32(y, l)
    rows = eng.attention_rows_long_f32(y, sorted(toks), layer)
    want = torch.stack([rows[:, sorted(toks).index(t)] for t in toks], dim=1).reshape(2, 3, th, tw)
    assert torch.equal(got, want)
    np.testing.assert_allclose(got.sum((-1, -2)).cpu().numpy(), 1.0, atol=1e-4)
    with pytest.raises(ValueError):
        eng.attention_map_long_f32(frames, th, tw, [(1, 1), (1, 1)], layer=layer)
    with pytest.raises(ValueError):
        eng.attention_map_long_f32(frames, th, tw, [(8, 0)], layer=layer)


def _refused(eng, status, S=256, rows=(0, 5), n_rows=None, want=TENSOR + ROW, seq_len=None, skew=0):
    """the call must raise with `status` and leave the canary-filled output and taps untouched; skew: bytes added to
    every tap pointer (the buffers are PAD bytes larger)"""
    import torch
    B, n = 1, len(rows)
    x = torch.zeros((B, S, eng.E), dtype=torch.float32, device="cuda")
    c = _canaries(eng, B, S, n, want, y=True)
    st = host._MhaLongF32Taps(**{k: c.ptr(k, skew) for k in want})
    arr = (host.C.c_int * max(n, 1))(*rows)
    st.rows, st.n_rows = (arr if n else None), (n if n_rows is None else n_rows)
    refused(lambda: _call(eng, x, c.views()["y"], st, seq_len), c, status)


def test_refusals_before_any_launch(engines):
    import torch
    for name in ("vitlstm_E64_seed0_B2", "onlyattn1l_E64_s0_B2"):          # ITAW0001, ITAW0002: int8 attention
        ei = host.Engine(long_case(name).blob, device=0)
        assert ei.attn_kind(0) == host.ATTN_INT8
        _refused(ei, UNSUPPORTED)
        assert "ita_mha_long_int8_taps" in host.lib().ita_error_string().decode()
        ei.close()
    eng = engines(64)
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
    for k in TENSOR:                                                     # 4-byte aligned is not enough: 16 bytes
        _refused(eng, INVALID, rows=(), want=(k,), skew=4)
    for k in ("logits", "probs"):
        _refused(eng, INVALID, rows=(0, 5), want=(k,), skew=8)
    for k in ("row_max", "row_sum"):
        _refused(eng, INVALID, rows=(0, 5), want=(k,), skew=2)
    # the handle then still runs a valid call correctly
    kind, (S, B) = "plain", lc.SHAPES[1]
    x = cu(lc.inputs(kind, 64, S, B))
    rows = ltc.rows_for(kind, 64, S, B, 0)
    y, got = eng.mha_long_f32_taps(x, rows)
    assert torch.equal(y, eng.mha_long_f32(x))
    _check_bounds(to_numpy(got), kind, 64, S, B, 0, rows)


def test_refused_inside_a_stream_capture(engines):
    import torch
    eng, kind, (S, B) = engines(64), "plain", lc.SHAPES[1]
    xc = cu(lc.inputs(kind, 64, S, B))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = eng.mha_long_f32(xc)                  # warm-up outside the capture: the workspace exists
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    y = torch.full_like(xc, SENTINEL)
    yg = torch.empty_like(xc)
    g = torch.cuda.CUDAGraph()
    message = None
    with torch.cuda.graph(g):
        host._chk(host.lib().ita_mha_long_f32(eng._h, 0, xc.data_ptr(), yg.data_ptr(), B, S, host._stream_ptr(eng.device)))
        try:
            _call(eng, xc, y, host._MhaLongF32Taps())
        except host.ITAError as e:
            message = str(e)
    assert message is not None and INVALID in message and "capture" in message, message
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(yg, out)
    assert bool((y == SENTINEL).all())
    del g
    rows = ltc.rows_for(kind, 64, S, B, 0)
    y2, got = eng.mha_long_f32_taps(xc, rows)
    assert torch.equal(y2, out)
    _check_bounds(to_numpy(got), kind, 64, S, B, 0, rows)
