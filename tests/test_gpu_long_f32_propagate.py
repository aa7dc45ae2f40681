"""Long float propagation on the MI355X: ita_mha_long_f32_propagate (Engine.attention_propagate_long_f32) and the attention
rollout built on it (attention_rollout_long_f32, attention_rollout_map_long_f32).  The cases, the weights, the references
and the bounds are those of long_f32_propagate_common.py, where they are derived; test_long_f32_propagate_cpu.py shows on
the CPU that an f32 model of the kernel stays inside them on every case here and that they reject six wrong kernels.

Shapes (S, B): (128, 3) one key tile and two query units, frames must stay apart; (256, 2) the ring wraps, two key tiles;
(384, 2) an odd tile count; (1024, 1) every row fits one taps call; (2048, 1) two taps calls.  All five input kinds at
S = 256, plain and ramp elsewhere.  Every case runs R = 64 rows (all ones, uniform, signed, all zero and six one-hot rows,
repeated); R = 1, 16 and 17 are held to the rows of the R = 64 call bit for bit.

Worst error / bound measured on the MI355X over all cases: against the kernels' own probabilities 0.036 (flat, E = 128,
S = 256; 0.002 at S = 2048); against float64 0.20 (ramp, E = 64, S = 256; from 0.08); the CPU model of the kernel gives the
same figures on every case.  Rollout against float64: 0.06 to 0.42 (E = 128, both layers, rows 200, 5, 130)."""
import numpy as np
import pytest

from drone_oa_iree_vit_accelerator_amd import attention_propagate_f32_ref as apr
from drone_oa_iree_vit_accelerator_amd import attention_rollout_f32_ref as arr
from drone_oa_iree_vit_accelerator_amd import host
from gpu_support import INVALID, UNSUPPORTED, Canaries, captured_replays, cu, engine_pool, refused
from long_cases import long_case
import long_f32_common as lc
import long_f32_propagate_common as pc
import long_f32_taps_common as ltc

pytestmark = pytest.mark.gpu

def _bits(t):
    import torch
    return t.contiguous().view(torch.int32)


def _same(a, b):
    import torch
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


@pytest.fixture(scope="module")
def engines():
    """(kind, E) -> Engine: the stock blob of E, or the flat one; opened on first use"""
    yield from engine_pool(lambda kind, E: pc.case(kind, E)[1], lambda kind, E: ("flat" if kind == "flat" else "stock", E))


def _call(eng, x, B, S, w, n_w, out, layer=0):
    """the raw C entry on device pointers (or None)"""
    host._chk(host.lib().ita_mha_long_f32_propagate(eng._h, layer, x, B, S, w, n_w, out, host._stream_ptr(eng.device)))


def _all_probs(eng, x):
    """the taps' probabilities of every query row (B, S, S), in calls of at most 1024 rows"""
    S = x.shape[1]
    return np.concatenate([eng.attention_rows_long_f32(x, list(range(r0, min(r0 + host.LONG_MAX_ROWS, S)))).cpu().numpy()
                           for r0 in range(0, S, host.LONG_MAX_ROWS)], axis=1)


@pytest.mark.parametrize("E", [64, 128])
@pytest.mark.parametrize("kind,S,B", pc.CASES)
def test_propagate_against_own_probabilities_and_float64(engines, kind, S, B, E):
    import torch
    eng = engines(kind, E)
    x, w = cu(pc.inputs(kind, E, S, B)), cu(pc.weights(S, B))
    got = eng.attention_propagate_long_f32(x, w)
    assert got.dtype == torch.float32 and tuple(got.shape) == (B, 64, S)
    assert torch.equal(x, cu(pc.inputs(kind, E, S, B))), "x was written to"
    assert torch.equal(w, cu(pc.weights(S, B))), "w was written to"
    g = got.cpu().numpy()
    assert np.isfinite(g).all()

    # 1. against the kernels' own probabilities: the gamma bound, one-hot rows the taps' bits, the zero row +0.0
    P = _all_probs(eng, x)
    bad, rt = pc.compare_taps(g, P, pc.weights(S, B))
    assert bad == []
    # 2. against float64 from the parameters, independent of any GPU value
    r64 = pc.ratio64(g, kind, E, S, B)
    print(f"{kind} E={E} S={S} B={B}: worst error / gamma bound {rt:.4f}, worst error / float64 bound {r64:.4f}; "
          f"(bound, e_torch) {pc.refs64(kind, E, S, B)[1:]}")
    assert r64 <= 1.0, r64
    # 3. the all-ones rows are attention received, up to the order of the additions
    cm = eng.attention_received_long_f32(x).double().cpu().numpy()
    for r in pc.rows_of("ones"):
        assert (np.abs(g[:, r] - cm) <= 2 * apr.gamma(S) * cm).all(), r
    # 4. row 37 alone has the bits it has among 64
    assert _same(eng.attention_propagate_long_f32(x, w[:, 37:38].contiguous()), got[:, 37:38])


@pytest.mark.parametrize("E", [64, 128])
def test_group_edges_and_canaries(engines, E):
    """R = 1, 16, 17, 64 into a canary-filled buffer of 64 rows and a tail: the rows are those of the R = 64 call, bit for
    bit, and nothing behind row R - 1 of the last frame is written"""
    import torch
    kind, S, B = "ramp", 256, 2
    eng = engines(kind, E)
    x, w = cu(pc.inputs(kind, E, S, B)), cu(pc.weights(S, B))
    full = eng.attention_propagate_long_f32(x, w)
    for R in pc.RS:
        wr = w[:, :R].contiguous()
        c = Canaries({"out": ((B, R, S), torch.float32)}, pad=4 * B * (64 - R) * S + 4096)
        _call(eng, x.data_ptr(), B, S, wr.data_ptr(), R, c.ptr("out"))
        torch.cuda.synchronize()
        assert _same(c.views()["out"], full[:, :R].contiguous()), R
        c.assert_untouched(written=("out",))
    # (R, S) weights: the same for every frame
    got = eng.attention_propagate_long_f32(x, w[1, :17])
    for b in range(B):
        assert _same(got[b:b + 1], eng.attention_propagate_long_f32(x[b:b + 1].contiguous(), w[1:2, :17].contiguous())), b
    for bad in (w[:, :, :128], w.double(), w.cpu(), w[:1]):
        with pytest.raises(host.ITAError, match="w must be an f32 GPU tensor"):
            eng.attention_propagate_long_f32(x, bad)


@pytest.mark.parametrize("E", [64, 128])
@pytest.mark.parametrize("S,B", [(128, 3), (256, 2), (384, 2)])
def test_same_bits_on_every_call_and_in_every_batch(engines, S, B, E):
    eng = engines("ramp", E)
    x, w = cu(pc.inputs("ramp", E, S, B)), cu(pc.weights(S, B)[:, :17])
    got = eng.attention_propagate_long_f32(x, w)
    assert _same(eng.attention_propagate_long_f32(x, w), got), "a second call gives other bits"
    flipped = eng.attention_propagate_long_f32(x.flip(0).contiguous(), w.flip(0).contiguous())
    assert _same(flipped.flip(0), got), "a frame's result depends on its place in the batch"
    for b in range(B):
        alone = eng.attention_propagate_long_f32(x[b:b + 1].contiguous(), w[b:b + 1].contiguous())
        assert _same(alone, got[b:b + 1]), f"frame {b} alone differs from frame {b} in the batch"


@pytest.mark.parametrize("E", [64, 128])
def test_production_path_undisturbed(engines, E):
    """the propagation shares the handle's workspace with mha_long_f32 and the statistics: neither disturbs the other"""
    import torch
    S, B = 256, 2
    eng = engines("plain", E)
    x, w = cu(pc.inputs("plain", E, S, B)), cu(pc.weights(S, B))
    y0 = eng.mha_long_f32(x)
    st0 = eng.attention_stats_long_f32(x)
    p0 = eng.attention_propagate_long_f32(x, w)
    assert torch.equal(_bits(eng.mha_long_f32(x)), _bits(y0))
    st1 = eng.attention_stats_long_f32(x)
    assert all(_same(st1[k], st0[k]) for k in st0)
    assert _same(eng.attention_propagate_long_f32(x, w), p0)


def test_captured_call_replays(engines):
    import torch
    S, B, E, R = 256, 2, 64, 17
    eng = engines("plain", E)
    x, w = cu(pc.inputs("plain", E, S, B)), cu(pc.weights(S, B)[:, :R])
    c = Canaries({"out": ((B, R, S), torch.float32)})
    captured_replays(lambda: {"out": eng.attention_propagate_long_f32(x, w)},
                     lambda: _call(eng, x.data_ptr(), B, S, w.data_ptr(), R, c.ptr("out")), c, ("out",))


def _refused(eng, status, S=256, seq_len=None, n_w=4, null=None, skew=None, layer=0):
    """the call must raise with `status` and leave the canary-filled output untouched"""
    import torch
    x = torch.zeros((1, S, eng.E), dtype=torch.float32, device="cuda")
    w = torch.ones((4 * S + 16,), dtype=torch.float32, device="cuda")
    c = Canaries({"out": ((1, 4, S), torch.float32)}, pad=32)
    args = dict(x=x.data_ptr(), w=w.data_ptr() + (4 if skew == "w" else 0), out=c.ptr("out", 4 if skew == "out" else 0))
    if null:
        args[null] = None
    refused(lambda: _call(eng, args["x"], 1, S if seq_len is None else seq_len, args["w"], n_w, args["out"], layer), c, status)


def test_refusals_before_any_launch(engines):
    for name in ("vitlstm_E64_seed0_B2", "onlyattn1l_E64_s0_B2"):          # ITAW0001, ITAW0002: int8 attention
        ei = host.Engine(long_case(name).blob, device=0)
        assert ei.attn_kind(0) == host.ATTN_INT8
        _refused(ei, UNSUPPORTED)
        assert "ita_mha_long_int8_propagate" in host.lib().ita_error_string().decode()
        x = cu(np.zeros((1, 256, ei.E), np.float32))
        with pytest.raises(host.ITAError, match="attention_rollout_long"):
            ei.attention_rollout_long_f32(x, [0])
        ei.close()
    eng = engines("plain", 64)
    _refused(eng, UNSUPPORTED, seq_len=200)
    _refused(eng, UNSUPPORTED, seq_len=0)
    _refused(eng, INVALID, n_w=0)
    _refused(eng, INVALID, n_w=65)
    _refused(eng, INVALID, layer=-1)
    _refused(eng, INVALID, layer=eng.num_layers)
    for null in ("w", "out", "x"):
        _refused(eng, INVALID, null=null)
    _refused(eng, INVALID, skew="w")
    _refused(eng, INVALID, skew="out")
    # the handle still runs, and a good call is what the kernels' own probabilities say
    S, B = 128, 3
    x = cu(pc.inputs("plain", 64, S, B))
    got = eng.attention_propagate_long_f32(x, cu(pc.weights(S, B))).cpu().numpy()
    assert pc.compare_taps(got, _all_probs(eng, x), pc.weights(S, B))[0] == []


# ---- rollout
def _rollout_refs(E, S, B, rows, first_layer):
    """(float64 rollout, bound, e_torch): rollout64 on float64 layer inputs, and torch's CPU f32 evaluation of the same
    recurrence on layer_torch's inputs"""
    import torch
    fp, _, twin = lc.case(E)
    nl = lc.LAYERS[E]
    x = lc.inputs("plain", E, S, B)
    xs64, xs32 = [x.astype(np.float64)], [x]
    for l in range(first_layer, nl - 1):
        xs64.append(lc.layer64(xs64[-1], fp, l))
        xs32.append(lc.layer_torch(twin, xs32[-1], l))
    want = arr.rollout64(xs64, fp, rows, first_layer)
    with torch.no_grad():
        F = torch.nn.functional
        v = torch.from_numpy(arr.start(B, S, rows).astype(np.float32))
        for l in range(nl - 1, first_layer - 1, -1):
            g = lambda n: torch.from_numpy(np.asarray(fp[f"attention_blocks.{l}.{n}"], np.float32).copy())
            xt = torch.from_numpy(np.array(xs32[l - first_layer], np.float32))
            q, k = F.linear(xt, g("q_proj.weight"), g("q_proj.bias")), F.linear(xt, g("k_proj.weight"), g("k_proj.bias"))
            v = 0.5 * (v + torch.matmul(v, torch.softmax(torch.matmul(q, k.transpose(-2, -1)), dim=-1)))
    e = float(np.abs(v.numpy() - want).max())
    return want, 3.0 * e + 4.0 * ltc.ulp32(np.abs(want).max()), e


@pytest.mark.parametrize("E,first_layer", [(64, 0), (128, 0), (128, 1)])
def test_rollout_against_float64(engines, E, first_layer):
    import torch
    S, B = 256, 2
    eng = engines("plain", E)
    assert eng.num_layers == lc.LAYERS[E]
    x = cu(lc.inputs("plain", E, S, B))
    for rows in ([200, 5, 130], None):          # key tiles 1, 0, 1; the single vector 1 / S
        got = eng.attention_rollout_long_f32(x, rows, first_layer)
        n = 3 if rows else 1
        assert got.dtype == torch.float32 and tuple(got.shape) == (B, n, S)
        g = got.double().cpu().numpy()
        assert (g >= 0).all() and (np.abs(g.sum(-1) - 1.0) <= 1e-4).all()
        want, bound, e = _rollout_refs(E, S, B, rows, first_layer)
        err = float(np.abs(g - want).max())
        print(f"rollout E={E} first_layer={first_layer} rows={rows}: error / bound {err / bound:.4f} (bound {bound:.3e}, e_torch {e:.3e})")
        assert err <= bound
    assert torch.equal(x, cu(lc.inputs("plain", E, S, B))), "x was written to"
    for bad in ([3, 3], [S], [-1]):
        with pytest.raises(ValueError):
            eng.attention_rollout_long_f32(x, bad)
    with pytest.raises(ValueError):
        eng.attention_rollout_long_f32(x, [0], first_layer=eng.num_layers)


def test_rollout_of_more_rows_than_a_call_takes(engines):
    """70 rows run as 64 + 6: bit for bit the rows computed in two calls"""
    S, B, E = 256, 2, 128
    eng = engines("plain", E)
    x = cu(lc.inputs("plain", E, S, B))
    rows = [int(r) for r in np.random.RandomState(7).permutation(S)[:70]]
    many = eng.attention_rollout_long_f32(x, rows)
    assert tuple(many.shape) == (B, 70, S)
    assert _same(many[:, :40], eng.attention_rollout_long_f32(x, rows[:40]))
    assert _same(many[:, 40:], eng.attention_rollout_long_f32(x, rows[40:]))


@pytest.mark.parametrize("E", [64, 128])
def test_attention_rollout_map_long_f32(engines, E):
    """u8 frames 120 x 180 on a 16 x 16 token grid (S = 256): tokenize_long, then attention_rollout_long_f32, reshaped,
    with the queries out of order"""
    import torch
    eng = engines("plain", E)
    frames = cu(np.random.RandomState(4).randint(0, 256, size=(2, 120, 180)).astype(np.uint8))
    queries = [(15, 15), (0, 0), (3, 9)]
    got = eng.attention_rollout_map_long_f32(frames, 16, 16, queries)
    assert tuple(got.shape) == (2, 3, 16, 16) and got.dtype == torch.float32
    y = eng.tokenize_long(frames, 16, 16)
    assert _same(got, eng.attention_rollout_long_f32(y, [ty * 16 + tx for ty, tx in queries]).reshape(2, 3, 16, 16))
    assert _same(eng.attention_rollout_map_long_f32(frames, 16, 16), eng.attention_rollout_long_f32(y).reshape(2, 1, 16, 16))
    assert float(got.min()) >= 0.0 and float(got[:, 1, 0, 0].min()) >= 0.5 ** eng.num_layers      # the identity residual
    for bad in ([(16, 0)], [(0, 16)], [(1, 1), (1, 1)]):
        with pytest.raises(ValueError):
            eng.attention_rollout_map_long_f32(frames, 16, 16, bad)
