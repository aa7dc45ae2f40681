"""The long-sequence entries on the MI355X at the sizes they are quoted and declared for: S = 8192 (B = 2), S = 65536
(B = 1, the most check_long_shape admits) and workspaces past 4 GiB.  Float attention, layer, taps and statistics against
the row-sampled float64 references of long_limits_common.py under the project's unchanged bounds (long_f32_common.bound,
the per-tensor rules of long_f32_taps_common and long_f32_stats_common; torch's own f32 error on the same rows sets them,
never GPU output); the int8 entries bit for bit against the oracle, long_taps_common.mha_rows and the class form of
attention_stats_ref.

Why these sizes.  With the stock weights a softmax row is one-hot, and a kernel that lost all but one 64-key unit would
pass at any length; the rows flattened by float_flat_common (q_proj times 0, 1 / 64, 1 / 8) make every unit count, and
at S = 8192 / 65536 there are 128 / 1024 units behind one another, 64 / 512 query tiles and a K ring that wraps hundreds
of times.  test_long_limits_cpu.py shows that one lost unit, or a ring one slot late, lands more than twice outside the
bound on these very rows at s = 0 and 1 / 64.  At s = 0 every probability is 1 / S exactly and all rows of a frame are
bit-equal, which is asserted on the whole output.

Rows: long_limits_common.rows_for(S) -- 0, 1, 127, 128, S/2 - 1, S/2, S - 129, S - 128, S - 1 and 55 seeded random ones.

Workspaces: 45 000 frames of S = 256 (int8: the V image starts at 4.42 GB of 6.7 GB) and of S = 128 (float: two images of
4.42 GB), gathered on the GPU from 61 distinct frames (a prime, so an offset that wraps at 2^32 bytes cannot land on a
copy of the same frame); the 61-frame call is held to the reference, the large one to it bit for bit.

Measured on an MI355X, worst err / bound: attention 0.28 (stock weights), 0.08 (s = 0, 1 / 64), 0.66 (s = 1 / 8); layer
0.43, 0.13, 0.72; taps 0.32; statistics 0.44.  row_gap on the flat vocabulary frame was 1.39 while the kernel added a
lane's S / 4 products in one chain; it sums a unit's 16 products first since ("Long float statistics")."""
import numpy as np
import pytest

from drone_oa_iree_vit_accelerator_amd import host
from drone_oa_iree_vit_accelerator_amd import mha_heads_ref as mref
from gpu_support import cu, engine_pool
import float_flat_common as fc
import long_f32_common as lc
import long_f32_stats_common as lsc
import long_f32_taps_common as ltc
import long_limits_common as ll
import long_taps_common as itc
from long_cases import long_case, long_f32, long_inputs

pytestmark = pytest.mark.gpu

GIB = 1 << 30
TENSOR, ROW = host.LONG_F32_TENSOR_TAPS, host.LONG_ROW_TAPS
VOCAB_F32 = (192, 64, 3)            # V, singles, seed of the float statistics' vocabulary frames
FRAMES, DISTINCT = 45000, 61


def _idx(rows):
    import torch
    return torch.tensor(list(rows), dtype=torch.long, device="cuda")


@pytest.fixture(scope="module")
def engines():
    yield from engine_pool(lambda E: lc.case(E)[1])


@pytest.fixture(scope="module")
def int8_refs():
    return dict(zip(ll.INT8_MODELS, ll.warm_int8()))


def _check(got, want, e_torch, what):
    """prints (err, e_torch), then asserts: every value finite, err within the rule's bound"""
    assert np.isfinite(got).all(), what
    err = float(np.abs(got - want).max())
    print(f"{what}: |gpu - float64| = {err:.3e}, |torch f32 - float64| = {e_torch:.3e}, ratio {err / e_torch:.2f}, "
          f"err / bound {err / lc.bound(e_torch):.2f}")
    assert err <= lc.bound(e_torch), (what, err, e_torch)


def _attention_and_layer(eng, kind, E, S, B, layer, s, what):
    """mha_long_f32 and encoder_layer_long_f32 (also with out aliasing x) on the sampled rows; returns the attention"""
    import torch
    rows, want_a, e_a, want_l, e_l = ll.ref(kind, E, S, B, layer, s)
    x, at = cu(lc.inputs(kind, E, S, B)), _idx(rows)
    y = eng.mha_long_f32(x, layer)
    assert bool(torch.isfinite(y).all()), what
    _check(y[:, at].cpu().numpy(), want_a, e_a, f"mha_long_f32 {what}")
    z = eng.encoder_layer_long_f32(x, layer)
    assert bool(torch.isfinite(z).all()), what
    _check(z[:, at].cpu().numpy(), want_l, e_l, f"encoder_layer_long_f32 {what}")
    alias = x.clone()
    assert eng.encoder_layer_long_f32(alias, layer, out=alias) is alias
    assert torch.equal(alias, z), f"{what}: out aliasing x"
    return x, y


# ---- float attention and layer
@pytest.mark.parametrize("S,B", ll.SIZES)
@pytest.mark.parametrize("E,layer", ll.MODELS)
@pytest.mark.parametrize("kind", ll.KINDS)
def test_attention_and_layer_against_float64(engines, kind, E, layer, S, B):
    _attention_and_layer(engines(E), kind, E, S, B, layer, 1, f"{kind} E={E} layer {layer} S={S} B={B}")


@pytest.mark.parametrize("S,B", ll.SIZES)
@pytest.mark.parametrize("E,layer", ll.MODELS)
@pytest.mark.parametrize("s", fc.SCALES, ids=fc.label)
def test_flat_rows_against_float64(E, layer, s, S, B):
    """q_proj times s: every one of the S / 64 units carries weight in every row.  At s = 0, on the whole output: every
    row of a frame bit-equal to row 0, and the taps' probabilities 1 / S exactly"""
    import torch
    eng = host.Engine(fc.case(E, layer, s)[1], device=0)
    for kind in fc.KINDS:
        x, y = _attention_and_layer(eng, kind, E, S, B, layer, s, f"s={fc.label(s)} {kind} E={E} layer {layer} S={S} B={B}")
        if s == 0:
            assert torch.equal(y, y[:, :1].expand_as(y)), (kind, "rows of a frame differ")
            tp = eng._long_f32_taps(x, ll.rows_for(S), layer, ("probs", "row_sum"))[1]
            assert bool((tp["probs"] == 1.0 / S).all()) and bool((tp["row_sum"] == float(S)).all()), kind
    eng.close()


@pytest.mark.parametrize("E,layer", ll.MODELS)
def test_frames_and_repeats(engines, E, layer):
    """bit for bit: frame b of a B = 2 call is the B = 1 call on that frame; two runs agree (S = 8192 and 65536)"""
    import torch
    eng = engines(E)
    for S, B in ll.SIZES:
        x = cu(lc.inputs("ramp", E, S, B))
        for f in (eng.mha_long_f32, eng.encoder_layer_long_f32):
            y = f(x, layer)
            assert torch.equal(y, f(x, layer)), (f.__name__, S)
            for b in range(B if B > 1 else 0):
                assert torch.equal(f(x[b:b + 1].contiguous(), layer)[0], y[b]), (f.__name__, S, b)


# ---- float taps
def _probs_from_taps(g, n):
    """the definition of the probs tap on the first n rows, each step rounded to f32"""
    inv = (np.float32(1.0) / g["row_sum"][:, :n]).astype(np.float32)
    return (ltc.expf((g["logits"][:, :n] - g["row_max"][:, :n, None]).astype(np.float32)) * inv[..., None]).astype(np.float32)


def _check_taps(eng, kind, E, S, B, layer, rows, want):
    import torch
    x = cu(lc.inputs(kind, E, S, B))
    y, got = eng._long_f32_taps(x, rows, layer, want)
    assert torch.equal(y, eng.mha_long_f32(x, layer))
    g = {k: v.cpu().numpy() for k, v in got.items()}
    t, r = ll.taps_ref(kind, E, S, B, layer, tuple(rows))
    bnd, err = ll.taps_bounds(t, r), ll.taps_errors(g, t, rows)
    assert set(err) == set(want) - {"row_max"}
    for k in err:
        print(f"taps {kind} E={E} layer {layer} S={S} B={B} n={len(rows)} {k}: |gpu - float64| = {err[k]:.3e}, e_torch {bnd[k][1]:.3e}, "
              f"bound {bnd[k][0]:.3e}, err / bound {err[k] / bnd[k][0]:.2f}")
    for k in err:
        assert np.isfinite(g[k]).all() and err[k] <= bnd[k][0], (k, err[k], bnd[k])
    np.testing.assert_array_equal(g["row_max"], g["logits"].max(-1))
    np.testing.assert_array_equal(g["probs"][:, :4], _probs_from_taps(g, 4))
    return got


@pytest.mark.parametrize("S,B", ll.SIZES)
@pytest.mark.parametrize("E,layer", ll.MODELS)
@pytest.mark.parametrize("kind", ["plain", "ramp"])
def test_taps_against_float64(engines, kind, E, layer, S, B):
    _check_taps(engines(E), kind, E, S, B, layer, ll.rows_for(S), TENSOR + ROW)


def test_taps_the_most_rows_at_the_longest_sequence(engines):
    """1024 rows of S = 65536, row 65535 among them: the row table's last entry, 256 MiB of logits"""
    import torch
    S, rows = 65536, ll.many_rows(65536)
    got = _check_taps(engines(64), "plain", 64, S, 1, 0, rows, ROW)
    few = engines(64)._long_f32_taps(cu(lc.inputs("plain", 64, S, 1)), ll.rows_for(S), 0, ROW)[1]
    at = _idx([rows.index(r) for r in ll.rows_for(S)])
    for k in ROW:
        assert torch.equal(few[k], got[k][:, at]), k


# ---- float statistics
@pytest.mark.parametrize("E", [64, 128])
@pytest.mark.parametrize("kind", ["plain", "ramp"])
@pytest.mark.parametrize("s", [1, 1.0 / 64], ids=fc.label)
def test_stats_at_8192_against_float64(kind, s, E):
    """the whole 8192 x 8192 matrix in float64 (formed 1024 query rows at a time); row_max and row_sum are the taps' bits"""
    import torch
    S = 8192
    t, bounds = ll.stats_ref(kind, E, S, s)
    eng = host.Engine(fc.case(E, 0, s)[1], device=0)
    x = cu(lc.inputs(kind, E, S, 1))
    st = eng.attention_stats_long_f32(x)
    for k in ("col_mass", "row_gap"):
        g = st[k].cpu().numpy()
        err = float(np.abs(g - t[k]).max())
        print(f"stats s={fc.label(s)} {kind} E={E} S={S} {k}: |gpu - float64| = {err:.3e}, e_torch {bounds[k][1]:.3e}, "
              f"bound {bounds[k][0]:.3e}, err / bound {err / bounds[k][0]:.2f}")
        assert np.isfinite(g).all() and err <= bounds[k][0], (k, err, bounds[k])
    assert float(st["col_mass"].sum(dtype=torch.float64)) == pytest.approx(S, rel=1e-5)
    rows = ll.rows_for(S)
    tp = eng._long_f32_taps(x, rows, 0, ("row_max", "row_sum"))[1]
    for k in ("row_max", "row_sum"):
        assert torch.equal(tp[k], st[k][:, _idx(rows)]), k
    eng.close()


@pytest.mark.parametrize("E", [64, 128])
@pytest.mark.parametrize("s", [1, 1.0 / 64], ids=fc.label)
def test_stats_at_65536_on_a_vocabulary_frame(s, E):
    """65536 tokens drawn from 192, 64 of them single (long_limits_common: vocabulary frames).  Every row statistic is
    bit-equal inside a class; with the taps of one row per class, long_f32_stats_common.compare holds row_max and row_sum
    to the taps' bits, row_nnz and col_nnz to counts @ (probs >= p_min) exactly and the sums to the gamma bounds; col_mass
    and row_gap are held to float64"""
    import torch
    S = 65536
    V, singles, seed = VOCAB_F32
    _, reps, cls, counts = ll.vocabulary(S, V, singles, seed)
    eng = host.Engine(fc.case(E, 0, s)[1], device=0)
    x = cu(ll.vocab_f32_frame(E, S, V, singles, seed))
    st = eng.attention_stats_long_f32(x)
    again = eng.attention_stats_long_f32(x)
    assert all(torch.equal(st[k], again[k]) for k in st)
    rep_at, cls_at = _idx(reps), _idx(cls)
    for k in ("row_max", "row_sum", "row_gap", "row_nnz"):
        assert torch.equal(st[k][0], st[k][0][rep_at][cls_at]), f"{k} differs inside a class"
    tp = {k: v.cpu().numpy() for k, v in eng._long_f32_taps(x, [int(r) for r in reps], 0, ROW)[1].items()}
    p = tp["probs"][0]
    keep = p >= np.float32(lsc.P_MIN)
    c = counts.astype(np.float64)
    ref = dict(row_max=tp["row_max"][:, cls], row_sum=tp["row_sum"][:, cls],
               row_nnz=keep.sum(-1).astype(np.int32)[cls][None], col_nnz=np.rint(c @ keep.astype(np.float64)).astype(np.int32)[None],
               col_mass=(c @ p.astype(np.float64))[None],
               row_gap=(p.astype(np.float64) * (tp["row_max"][0].astype(np.float64)[:, None] - tp["logits"][0].astype(np.float64))).sum(-1)[cls][None])
    got = {k: v.cpu().numpy() for k, v in st.items()}
    assert lsc.compare(got, ref, S) == []
    t, bounds = ll.vocab_stats_ref(E, S, V, singles, seed, s)
    for k in ("col_mass", "row_gap"):
        err = float(np.abs(got[k] - t[k]).max())
        print(f"stats s={fc.label(s)} vocabulary E={E} S={S} {k}: |gpu - float64| = {err:.3e}, e_torch {bounds[k][1]:.3e}, "
              f"bound {bounds[k][0]:.3e}, err / bound {err / bounds[k][0]:.2f}")
        assert np.isfinite(got[k]).all() and err <= bounds[k][0], (k, err, bounds[k])
    eng.close()


# ---- int8 at S = 65536
@pytest.mark.parametrize("name,l", ll.INT8_MODELS)
def test_int8_sampled_rows_at_65536(oracle, name, l):
    """mha_long_q8 and mha_long against oracle.mha_q8_rows and its dequantised rows; where the fixture has a layer,
    encoder_layer_long against the oracle composition on those rows (LayerNorm and the FFN are per token)"""
    import torch
    S = 65536
    case = long_case(name)
    E, t, fp, blob = case.E, case.t, case.fp, case.blob
    rows = ll.rows_for(S)
    at = _idx(rows)
    xq = long_inputs(S + l, 1, S, E)
    x = long_f32(S + l, 1, S, E, t, l)
    want_q = oracle.mha_q8_rows(xq[0], t, rows, l)
    assert len({r.tobytes() for r in want_q}) > len(rows) // 2
    eng = host.Engine(blob, device=0)
    got_q = eng.mha_long_q8(cu(xq), l)
    np.testing.assert_array_equal(got_q[0, at].cpu().numpy(), want_q, err_msg=name)
    assert torch.equal(got_q, eng.mha_long_q8(cu(xq), l))
    xc = cu(x)
    want_a = want_q.astype(np.float32) * np.float32(t[f"attn{l}.scal"][mref.SO])
    np.testing.assert_array_equal(eng.mha_long(xc, l)[0, at].cpu().numpy(), want_a, err_msg=name)
    if fp is not None:
        xr = x[:, list(rows)]
        x1 = oracle.add_ln(xr, want_a[None], fp[f"norms1.{l}.weight"], fp[f"norms1.{l}.bias"])
        want = oracle.add_ln(x1, oracle.ffn(x1, t, l), fp[f"norms2.{l}.weight"], fp[f"norms2.{l}.bias"])
        got = eng.encoder_layer_long(xc, l)
        np.testing.assert_array_equal(got[:, at].cpu().numpy(), want, err_msg=f"{name} layer {l}")
        alias = xc.clone()
        eng.encoder_layer_long(alias, l, out=alias)
        assert torch.equal(alias, got)
    eng.close()


@pytest.mark.parametrize("name,l", ll.INT8_MODELS)
def test_int8_taps_and_stats_at_65536(int8_refs, name, l):
    """a vocabulary frame of 512 tokens, 256 of them single: mha_long_taps with 1024 rows (the representatives, row 65535
    among them) against long_taps_common.mha_rows, attention_stats_long against the class form; every output bit for bit"""
    x, rows, want, stats = int8_refs[(name, l)]
    S = x.shape[1]
    eng = host.Engine(long_case(name).blob, device=0)
    xc, at = cu(x), _idx(rows)
    _, tp = eng.mha_long_taps(xc, rows, l)
    for k in ("logits", "probs"):
        np.testing.assert_array_equal(tp[k].cpu().numpy(), want[k], err_msg=f"{name} layer {l} {k}")
    for k in ("ctx", "out_q"):
        np.testing.assert_array_equal(tp[k][:, at].cpu().numpy(), want[k], err_msg=f"{name} layer {l} {k}")
    np.testing.assert_array_equal(tp["row_max"].cpu().numpy(), want["logits"].max(-1))
    np.testing.assert_array_equal(tp["row_sum"].cpu().numpy(), itc.row_sums(want["logits"]))
    got = eng.attention_stats_long(xc, l)
    assert tuple(got) == host.LONG_STATS
    for k, v in stats.items():
        g = got[k].cpu().numpy()
        assert g.dtype == v.dtype and g.shape == v.shape == (1, S), k
        np.testing.assert_array_equal(g, v, err_msg=f"{name} layer {l} {k}")
    eng.close()


# ---- workspaces past 4 GiB
def _room(need_gib, what):
    import torch
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info()[0]
    assert free >= need_gib * GIB, f"{what} needs {need_gib} GiB of device memory, {free / GIB:.1f} GiB are free"


def _gathered(small_in, call):
    """(the large call's output, the small call's output gathered the same way): 45 000 frames, frame b a copy of b % 61"""
    import torch
    pick = torch.arange(FRAMES, device="cuda") % DISTINCT
    small = call(small_in)
    big = call(small_in[pick].contiguous())
    return big, small, pick


def _same_frames(big, small, pick):
    """with torch on the device: every frame of the large call has the bits of the frame it is a copy of"""
    import torch
    same = (big == small[pick]).flatten(1).all(1)
    assert bool(same.all()), f"frames {torch.nonzero(~same).flatten()[:8].tolist()} differ from their copies"


def test_int8_workspace_past_4_gib(oracle):
    """mha_long_q8, E = 64, S = 256: 90 000 tiles, Q fragments, K and V images of 2.2 GB each, the V image past 2^32 bytes"""
    import torch
    _room(10, "the int8 case")
    case = long_case("blocks_E64_seed2_B1")
    E, t, blob = case.E, case.t, case.blob
    base = long_inputs(61, DISTINCT, 256, E)
    eng = host.Engine(blob, device=0)
    big, small, pick = _gathered(cu(base), eng.mha_long_q8)
    np.testing.assert_array_equal(small.cpu().numpy(), oracle.mha_q8(base, t))
    assert len({f.tobytes() for f in small.cpu().numpy()}) == DISTINCT
    assert tuple(big.shape) == (FRAMES, 256, E)
    _same_frames(big, small, pick)
    del big, small
    eng.close()
    torch.cuda.empty_cache()


def test_float_workspace_past_4_gib():
    """mha_long_f32, E = 64, S = 128: K and V images of 4.42 GB each"""
    import torch
    _room(14, "the float case")
    kind, E, S = "plain", 64, 128
    want, e_torch = lc.attn_ref(kind, E, S, DISTINCT, 0)
    eng = host.Engine(lc.case(E)[1], device=0)
    big, small, pick = _gathered(cu(lc.inputs(kind, E, S, DISTINCT)), eng.mha_long_f32)
    _check(small.cpu().numpy(), want, e_torch, f"mha_long_f32 {kind} E={E} S={S} B={DISTINCT}")
    assert tuple(big.shape) == (FRAMES, S, E)
    _same_frames(big.view(torch.int32), small.view(torch.int32), pick)
    del big, small
    eng.close()
    torch.cuda.empty_cache()
