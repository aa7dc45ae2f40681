"""Long-sequence propagation on the MI355X: ita_mha_long_int8_propagate (Engine.attention_propagate_long) against the
numpy definition attention_propagate_ref, and the attention rollout built on it (Engine.attention_rollout_long,
attention_rollout_map_long) against attention_rollout_ref.  Every comparison is an equality.

Shapes: S = 128 one query tile, 256 both ring slots, 384 an odd tile count, 1024 many tiles; B = 1 and 3 with frames and
weights that differ per frame; R = 1, 16, 17 (one row in the second group of 16, fifteen masked) and 64.  Weights:
long_propagate_common.weights.  At S = 8192 and 65536 the entry is held to entries that earlier tests hold to the
definition: attention_received_long and attention_rows_long."""
import numpy as np
import pytest

from drone_oa_iree_vit_accelerator_amd import attention_rollout_ref as arr
from drone_oa_iree_vit_accelerator_amd import host, params, synth
from heads_common import FIX_HEADS_2L, case as heads_case
import long_propagate_common as lpc
from gpu_support import INVALID, UNSUPPORTED, Canaries, cu, refused
from long_cases import long_case, tokens

pytestmark = pytest.mark.gpu

def _engine(name):
    _, _, blob = lpc.blob_case(name)
    eng = host.Engine(blob, device=0)
    forms = eng.layer_forms(0)
    assert forms["attn_image"], (name, forms)
    if name in lpc.CRAFTED:
        assert forms["fast"] == (name == "fast"), forms
    return eng


@pytest.mark.parametrize("S", lpc.SEQS)
@pytest.mark.parametrize("name", lpc.BLOBS)
def test_propagate_equals_the_definition(name, S):
    import torch
    x, w, want = lpc.expected(name, S)
    eng = _engine(name)
    for B in lpc.BATCHES:
        xc = cu(x[:B])
        for R in lpc.ROWS:
            got = eng.attention_propagate_long(xc, cu(w[:B, :R]))
            assert got.dtype == torch.int32 and tuple(got.shape) == (B, R, S)
            np.testing.assert_array_equal(got.cpu().numpy(), want[:B, :R], err_msg=f"{name} S={S} B={B} R={R}")
        assert torch.equal(xc, cu(x[:B])), "x was written to"
    # (R, S) weights: the same for every frame
    got = eng.attention_propagate_long(cu(x), cu(w[1, :17]))
    for b in range(3):
        one = eng.attention_propagate_long(cu(x[b:b + 1]), cu(w[1:2, :17]))
        assert torch.equal(got[b:b + 1], one), b
    eng.close()


@pytest.mark.parametrize("name", lpc.FIXTURES)
def test_frames_and_repeats(name):
    """a call with B = 3 equals three calls with B = 1; a call repeated gives the same bytes"""
    import torch
    S = 384
    x, w, want = lpc.expected(name, S)
    eng = _engine(name)
    xc, wc = cu(x), cu(w)
    got = eng.attention_propagate_long(xc, wc)
    for b in range(3):
        assert torch.equal(eng.attention_propagate_long(xc[b:b + 1].contiguous(), wc[b:b + 1].contiguous()), got[b:b + 1]), b
    assert torch.equal(eng.attention_propagate_long(xc, wc), got)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    eng.close()


@pytest.mark.parametrize("S", [8192, 65536])
@pytest.mark.parametrize("name", lpc.FIXTURES)
def test_identities_at_long_sequences(name, S):
    """one frame, R = 18: the ones row is attention_received_long, the minus-ones row its negative, sixteen one-hot rows
    (tile borders and the last token among them) are attention_rows_long of those rows"""
    import torch
    E, t, _ = lpc.blob_case(name)
    eng = _engine(name)
    xc = cu(tokens(S + 1, 1, S, E, t))
    fixed = {0, 127, 128, 129, S // 2 - 1, S // 2, S - 129, S - 128, S - 1}
    extra = [int(r) for r in np.random.RandomState(S).permutation(S) if int(r) not in fixed][:16 - len(fixed)]
    rows = sorted(fixed | set(extra))
    assert len(rows) == 16
    w = np.zeros((1, 18, S), np.int8)
    w[0, 0], w[0, 1] = 1, -1
    for n, r in enumerate(rows):
        w[0, 2 + n, r] = 1
    got = eng.attention_propagate_long(xc, cu(w))
    received = eng.attention_received_long(xc)
    assert torch.equal(got[:, 0], received) and torch.equal(got[:, 1], -received)
    assert int(received.max()) > 0
    assert torch.equal(got[:, 2:], eng.attention_rows_long(xc, rows).to(torch.int32))
    eng.close()


def _call(eng, x, w, out, n_w, S=None, B=1):
    ptr = lambda t: t if isinstance(t, int) or t is None else t.data_ptr()
    host._chk(host.lib().ita_mha_long_int8_propagate(eng._h, 0, ptr(x), B, x.shape[1] if S is None else S, ptr(w), n_w, ptr(out),
                                                     host._stream_ptr(eng.device)))


def _refused(eng, status, S=256, seq_len=None, n_w=4, null=None, skew=None):
    """the call must raise with `status` and leave the canary-filled output untouched"""
    import torch
    x = torch.zeros((1, S, eng.E), dtype=torch.float32, device="cuda")
    w = torch.ones((4 * S + 16,), dtype=torch.int8, device="cuda")
    c = Canaries({"out": ((1, 4, S), torch.int32)}, pad=32)
    args = dict(x=x, w=w.data_ptr() + (2 if skew == "w" else 0), out=c.ptr("out", 4 if skew == "out" else 0))
    if null:
        args[null] = None
    refused(lambda: _call(eng, args["x"], args["w"], args["out"], n_w, S if seq_len is None else seq_len), c, status)


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
    eng = _engine(name)
    _refused(eng, UNSUPPORTED, seq_len=200)
    _refused(eng, UNSUPPORTED, seq_len=0)
    _refused(eng, INVALID, n_w=0)
    _refused(eng, INVALID, n_w=65)
    for null in ("w", "out", "x"):
        _refused(eng, INVALID, null=null)
    _refused(eng, INVALID, skew="w")
    _refused(eng, INVALID, skew="out")
    x, w, want = lpc.expected(name, 256)
    np.testing.assert_array_equal(eng.attention_propagate_long(cu(x), cu(w)).cpu().numpy(), want, err_msg="after the refusals")
    eng.close()


def test_captured_call_replays():
    """one eager call (the workspace is held), then the call captured on one stream and replayed twice, with x and w
    rewritten between the replays"""
    import torch
    name, S, B, R = "vitlstm_E64_seed0_B2", 256, 3, 17
    x, w, want = lpc.expected(name, S)
    eng = _engine(name)
    xc, wc = cu(x), cu(w[:, :R])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = eng.attention_propagate_long(xc, wc)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(eager.cpu().numpy(), want[:, :R], err_msg="eager")
    c = Canaries({"out": ((B, R, S), torch.int32)})
    out = c.views()["out"]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _call(eng, xc, wc, out, R, B=B)
    g.replay()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), want[:, :R], err_msg="first replay")
    c.assert_untouched(written=("out",))
    # the frames in another order, other weight rows
    order = [2, 0, 1]
    xc.copy_(cu(x[order]))
    wc.copy_(cu(w[order, 40:40 + R]))
    c.refill()
    g.replay()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), want[order, 40:40 + R], err_msg="second replay")
    c.assert_untouched(written=("out",))
    del g
    eng.close()


@pytest.mark.parametrize("name", lpc.ROLLOUT_BLOBS)
def test_rollout_equals_the_definition(oracle, name):
    import torch
    case = long_case(name)
    E, nl, t, fp, blob = case.E, case.num_layers, case.t, case.fp, case.blob
    assert nl == (2 if name.startswith("vit2l") else 1)
    S, B = 256, 2
    x = tokens(S + B, B, S, E, t)
    eng = host.Engine(blob, device=0)
    xc = cu(x)
    for rows in ((0, 100, 255), None):
        got = eng.attention_rollout_long(xc, rows)
        want = arr.rollout(oracle, x, t, fp, nl, rows)
        assert got.dtype == torch.float64 and tuple(got.shape) == want.shape == (B, 3 if rows else 1, S)
        np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=f"{name} rows={rows}")
    if nl == 2:      # from the second layer on: x enters layer 1
        got = eng.attention_rollout_long(xc, (5, 3), first_layer=1)
        np.testing.assert_array_equal(got.cpu().numpy(), arr.rollout(oracle, x, t, fp, nl, (5, 3), first_layer=1))
    # 22 rows: two chunks; the same rows one at a time
    rows = [int(r) for r in np.random.RandomState(7).permutation(S)[:22]]
    many = eng.attention_rollout_long(xc, rows)
    assert tuple(many.shape) == (B, 22, S)
    for n, r in enumerate(rows):
        assert torch.equal(many[:, n:n + 1], eng.attention_rollout_long(xc, [r])), (n, r)
    with pytest.raises(ValueError):
        eng.attention_rollout_long(xc, [3, 3])
    with pytest.raises(ValueError):
        eng.attention_rollout_long(xc, [S])
    assert torch.equal(xc, cu(x)), "x was written to"
    eng.close()


def test_attention_rollout_map_long():
    """u8 frames 60 x 90 -> an 8 x 16 token grid on the two-layer E = 128 blob: tokenize_long plus attention_rollout_long,
    reshaped, with the queries out of order"""
    import torch
    eng = host.Engine(long_case("vit2l_E128_s0_B2").blob, device=0)
    frames = cu(np.random.RandomState(4).randint(0, 256, size=(2, 60, 90)).astype(np.uint8))
    queries = [(7, 15), (0, 0), (3, 9)]
    got = eng.attention_rollout_map_long(frames, 8, 16, queries)
    assert tuple(got.shape) == (2, 3, 8, 16) and got.dtype == torch.float64
    y = eng.tokenize_long(frames, 8, 16)
    assert torch.equal(got, eng.attention_rollout_long(y, [ty * 16 + tx for ty, tx in queries]).reshape(2, 3, 8, 16))
    assert torch.equal(eng.attention_rollout_map_long(frames, 8, 16), eng.attention_rollout_long(y).reshape(2, 1, 8, 16))
    assert float(got.min()) >= 0.0 and float(got[:, 1, 0, 0].min()) >= 0.25      # the identity residual of both layers
    for bad in ([(8, 0)], [(0, 16)], [(1, 1), (1, 1)]):
        with pytest.raises(ValueError):
            eng.attention_rollout_map_long(frames, 8, 16, bad)
    eng.close()
