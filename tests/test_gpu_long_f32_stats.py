"""Long float attention statistics on the MI355X: ita_mha_long_f32_stats (Engine.attention_stats_long_f32,
attention_received_long_f32, attention_received_map_long_f32).  The cases, the references and the bounds are those of
long_f32_stats_common.py, where they are derived; test_long_f32_stats_cpu.py shows on the CPU that an f32 model of the
kernel stays inside them on every case here and that they reject six wrong kernels.

Shapes (S, B): (128, 3) one query tile and two units, frames must stay apart; (256, 2) two tiles and four units: the ring
wraps, partials of two tiles; (384, 2) an odd tile count; (1024, 1) every row fits one taps call; (2048, 1) two taps
calls of 1024 rows and 16 tiles of partials.  All five input kinds at S = 256, plain and ramp elsewhere.

Worst error / bound against float64 measured on the MI355X over all cases: col_mass 0.23 (plain, E = 128, S = 128),
row_gap 0.27 (ramp, E = 64, S = 256); the CPU model of the kernel gives the same figures on every case."""
import numpy as np
import pytest
import torch

from drone_oa_iree_vit_accelerator_amd import attention_stats_f32_ref as asr
from drone_oa_iree_vit_accelerator_amd import host
from gpu_support import INVALID, UNSUPPORTED, Canaries, captured_replays, cu, engine_pool, refused, same_bits, to_numpy
from long_cases import long_case
import long_f32_common as lc
import long_f32_stats_common as sc

pytestmark = pytest.mark.gpu

STATS = host.LONG_F32_STATS
ROW_TAPS = ("logits", "row_max", "row_sum")


@pytest.fixture(scope="module")
def engines():
    """(kind, E) -> Engine: the stock blob of E, or the flat one; opened on first use"""
    yield from engine_pool(lambda kind, E: sc.case(kind, E)[1], lambda kind, E: ("flat" if kind == "flat" else "stock", E))


def _taps_of_all_rows(eng, x):
    """logits (B, S, S), row_max, row_sum (B, S) of every query row, in taps calls of at most 1024 rows"""
    S = x.shape[1]
    parts = [to_numpy(eng._long_f32_taps(x, list(range(r0, min(r0 + host.LONG_MAX_ROWS, S))), 0, ROW_TAPS)[1])
             for r0 in range(0, S, host.LONG_MAX_ROWS)]
    return {k: np.concatenate([p[k] for p in parts], axis=1) for k in ROW_TAPS}


@pytest.mark.parametrize("E", [64, 128])
@pytest.mark.parametrize("kind,S,B", sc.CASES)
def test_stats_against_own_probabilities_and_float64(engines, kind, S, B, E):
    eng = engines(kind, E)
    x = cu(sc.inputs(kind, E, S, B))
    got = eng.attention_stats_long_f32(x)
    assert tuple(got) == STATS + ("row_entropy",)
    for k, v in got.items():
        assert tuple(v.shape) == (B, S) and v.dtype == (torch.int32 if k.endswith("_nnz") else torch.float32), k
    assert torch.equal(x, cu(sc.inputs(kind, E, S, B))), "x was written to"
    assert torch.equal(got["row_entropy"], torch.log(got["row_sum"]) + got["row_gap"])
    g = to_numpy(got)
    assert all(np.isfinite(g[k]).all() for k in g) and (g["row_gap"] >= 0).all()

    # 1. against the kernels' own probabilities
    tp = _taps_of_all_rows(eng, x)
    ref = asr.stats_from_taps(tp["logits"], tp["row_max"], tp["row_sum"], sc.P_MIN)
    assert sc.compare(g, ref, S) == []
    P = ref["probs"]
    inside = P[(P > 1e-3) & (P < 0.5)]
    occurring = float(np.sort(inside)[len(inside) // 2])       # a boundary that sits on a value P holds
    assert (P == np.float32(occurring)).any()
    for p_min in (1.0 / 16, occurring):
        c = to_numpy(eng._long_f32_stats(x, 0, ("row_nnz", "col_nnz"), p_min))
        keep = P >= np.float32(p_min)
        np.testing.assert_array_equal(c["row_nnz"], keep.sum(-1), err_msg=f"row_nnz at p_min = {p_min!r}")
        np.testing.assert_array_equal(c["col_nnz"], keep.sum(-2), err_msg=f"col_nnz at p_min = {p_min!r}")
    assert (np.abs(g["col_mass"].astype(np.float64).sum(-1) - S) <= 1e-4 * S).all()

    # 2. against float64, independent of the taps
    ratios = sc.ratios64(g, kind, E, S, B)
    t = sc.refs64(kind, E, S, B)
    print(f"{kind} E={E} S={S} B={B}: worst error / bound against float64 {ratios}; (bound, e_torch) col_mass "
          f"{t['bound_col_mass']}, row_gap {t['bound_row_gap']}")
    assert max(ratios.values()) <= 1.0, ratios
    if kind == "spike_last":
        assert (g["col_mass"][:, S - 1] > S / 8).all() and (g["row_gap"] < 1e-6).mean() > 0.1


@pytest.mark.parametrize("E", [64, 128])
@pytest.mark.parametrize("S,B", [(128, 3), (256, 2), (384, 2)])
def test_same_bits_on_every_call_and_in_every_batch(engines, S, B, E):
    eng = engines("ramp", E)
    x = cu(sc.inputs("ramp", E, S, B))
    got = eng._long_f32_stats(x, 0, STATS, sc.P_MIN)
    assert same_bits(eng._long_f32_stats(x, 0, STATS, sc.P_MIN), got, STATS), "a second call gives other bits"
    flipped = eng._long_f32_stats(x.flip(0).contiguous(), 0, STATS, sc.P_MIN)
    assert same_bits({k: v.flip(0) for k, v in flipped.items()}, got, STATS), "a frame's result depends on its place in the batch"
    for b in range(B):
        alone = eng._long_f32_stats(x[b:b + 1].contiguous(), 0, STATS, sc.P_MIN)
        assert same_bits(alone, {k: v[b:b + 1] for k, v in got.items()}, STATS), f"frame {b} alone differs from frame {b} in the batch"


def _canaries(B, S):
    return Canaries({k: ((B, S), torch.int32 if k.endswith("_nnz") else torch.float32) for k in STATS})


def _call(eng, x, st, S=None, p_min=sc.P_MIN):
    host._chk(host.lib().ita_mha_long_f32_stats(eng._h, 0, x.data_ptr() if x is not None else None, 1 if x is None else x.shape[0],
                                                (256 if x is None else x.shape[1]) if S is None else S, p_min,
                                                host.C.byref(st) if st is not None else None, host._stream_ptr(eng.device)))


@pytest.mark.parametrize("E", [64, 128])
def test_each_statistic_alone(engines, E):
    """asked for alone a statistic has the bits of the full call, and what is not asked for is not written"""
    S, B = 384, 2
    eng = engines("plain", E)
    x = cu(sc.inputs("plain", E, S, B))
    full = eng._long_f32_stats(x, 0, STATS, sc.P_MIN)
    assert torch.equal(eng.attention_received_long_f32(x), full["col_mass"])
    for want in [(k,) for k in STATS] + [("row_max", "row_sum"), ("row_gap", "row_nnz"), ("col_mass", "col_nnz")]:
        c = _canaries(B, S)
        _call(eng, x, host._MhaLongF32Stats(**c.ptrs(want)))
        torch.cuda.synchronize()
        assert same_bits(c.views(), full, want), want
        c.assert_untouched(written=want)


@pytest.mark.parametrize("E", [64, 128])
def test_production_path_undisturbed(engines, E):
    """the statistics share the handle's workspace with mha_long_f32 and its taps: neither disturbs the other"""
    S, B = 256, 2
    eng = engines("plain", E)
    x = cu(sc.inputs("plain", E, S, B))
    y0 = eng.mha_long_f32(x)
    st0 = eng._long_f32_stats(x, 0, STATS, sc.P_MIN)
    assert torch.equal(eng.mha_long_f32(x), y0)
    assert same_bits(eng._long_f32_stats(x, 0, STATS, sc.P_MIN), st0, STATS)
    y1, _ = eng.mha_long_f32_taps(x, [0, 200])
    assert torch.equal(y1, y0)
    assert same_bits(eng._long_f32_stats(x, 0, STATS, sc.P_MIN), st0, STATS)


def test_captured_call_replays(engines):
    S, B, E = 256, 2, 64
    eng = engines("plain", E)
    x = cu(sc.inputs("plain", E, S, B))
    c = _canaries(B, S)
    st = host._MhaLongF32Stats(**c.ptrs())
    captured_replays(lambda: eng._long_f32_stats(x, 0, STATS, sc.P_MIN), lambda: _call(eng, x, st), c, STATS)


def _refused(eng, status, S=256, seq_len=None, null_x=False, want=STATS, skew=None, p_min=sc.P_MIN):
    """the call must raise with `status` and leave the canary-filled outputs untouched"""
    x = torch.zeros((1, S, eng.E), dtype=torch.float32, device="cuda")
    c = _canaries(1, S)
    st = host._MhaLongF32Stats(**{k: c.ptr(k, 2 if k == skew else 0) for k in want})
    refused(lambda: _call(eng, None if null_x else x, st, S if seq_len is None else seq_len, p_min), c, status)


def test_refusals_before_any_launch(engines):
    for name in ("vitlstm_E64_seed0_B2", "onlyattn1l_E64_s0_B2"):          # ITAW0001, ITAW0002: int8 attention
        ei = host.Engine(long_case(name).blob, device=0)
        assert ei.attn_kind(0) == host.ATTN_INT8
        _refused(ei, UNSUPPORTED)
        assert "ita_mha_long_int8_stats" in host.lib().ita_error_string().decode()
        ei.close()
    eng = engines("plain", 64)
    _refused(eng, UNSUPPORTED, seq_len=200)
    _refused(eng, UNSUPPORTED, seq_len=0)
    _refused(eng, INVALID, null_x=True)
    _refused(eng, INVALID, want=())
    _refused(eng, INVALID, skew="col_mass")
    for p_min in (0.0, -1.0, 1.5, float("nan")):
        _refused(eng, INVALID, p_min=p_min)
    # the handle still runs, and a good call is what the kernels' own probabilities say
    S, B = 128, 3
    x = cu(sc.inputs("plain", 64, S, B))
    tp = _taps_of_all_rows(eng, x)
    ref = asr.stats_from_taps(tp["logits"], tp["row_max"], tp["row_sum"], sc.P_MIN)
    assert sc.compare(to_numpy(eng._long_f32_stats(x, 0, STATS, sc.P_MIN)), ref, S) == []


@pytest.mark.parametrize("E,layer", [(64, 0), (128, 1)])
def test_attention_received_map_long_f32(engines, E, layer):
    """u8 frames 120 x 180 on a 16 x 16 token grid (S = 256): the composition of tokenize_long, the float encoder layers
    below `layer` and attention_received_long_f32"""
    eng = engines("plain", E)
    assert eng.num_layers == lc.LAYERS[E] > layer
    frames = cu(np.random.RandomState(4).randint(0, 256, size=(2, 120, 180)).astype(np.uint8))
    got = eng.attention_received_map_long_f32(frames, 16, 16, layer=layer)
    assert tuple(got.shape) == (2, 16, 16) and got.dtype == torch.float32
    y = eng.tokenize_long(frames, 16, 16)
    for l in range(layer):
        y = eng.encoder_layer_long_f32(y, l)
    want = eng.attention_received_long_f32(y, layer).reshape(2, 16, 16)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert (np.abs(got.double().sum((1, 2)).cpu().numpy() - 256) <= 1e-4 * 256).all()
    with pytest.raises(ValueError):
        eng.attention_received_map_long_f32(frames, 16, 16, layer=eng.num_layers)
