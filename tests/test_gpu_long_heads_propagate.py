"""Per-head weighted column sums and rollout of the long int8 attention on the MI355X: ita_mha_long_heads_int8_propagate
(Engine.attention_propagate_long_heads, attention_rollout_long_heads; csrc/ita_long_heads_prop_kernel.h), every sum equal
to attention_propagate_heads_ref.propagate_heads and the rollout to attention_rollout_heads_ref.rollout.  The kernels are
integer and the rollout's float64 steps are single roundings: every comparison is an equality.

Weights and inputs are test_gpu_long_heads_stats.py's: the E = 64, H = 3 fixture and layer 0 of the E = 128, H = 4
two-layer fixture, packed with the head count under test; long_cases.long_f32, seed 5.  The E = 64 fixture selects the FAST
(single-rounding) instantiations of the kernels and the E = 128 fixture the exact ones.  Weight rows are
long_propagate_common.weights(S, 3); the sums are linear in the rows, so the first R rows of one definition per (E, H, S)
serve every R."""
import functools

import numpy as np
import pytest
import torch

import long_propagate_common as lpc
from drone_oa_iree_vit_accelerator_amd import attention_rollout_heads_ref as arhr
from drone_oa_iree_vit_accelerator_amd import host, params, synth
from drone_oa_iree_vit_accelerator_amd.attention_propagate_heads_ref import propagate_heads
from gpu_support import INVALID, UNSUPPORTED, Canaries, cu, engine_pool, refused
from heads_common import FIX_HEADS, FIX_HEADS_2L, case, heads_of
from long_cases import long_f32

pytestmark = pytest.mark.gpu

SEED = 5
FIXTURE = {64: [p for p in FIX_HEADS if heads_of(p) == 3][0], 128: FIX_HEADS_2L[0]}


@functools.lru_cache(maxsize=None)
def blob(E, H):
    d, _, _, nl, _, fp, _ = case(FIXTURE[E])
    return params.blob_from_record(d, fp, E=E, num_layers=nl, H=H)


@pytest.fixture(scope="module")
def engines():
    yield from engine_pool(blob)


@functools.lru_cache(maxsize=None)
def reference(E, H, S):
    """(x (3, S, E), w (3, 64, S), propagate_heads of them (3, H, 64, S)); read-only"""
    t = case(FIXTURE[E])[4]
    x, w = long_f32(SEED, 3, S, E, t), lpc.weights(S, 3)
    want = propagate_heads(x, t, w, H)
    for a in (x, w, want):
        a.setflags(write=False)
    return x, w, want


def raw_call(eng, x, w, out, n_w, S=None):
    """the C entry on device tensors or raw addresses (None: NULL)"""
    ptr = lambda t: t if isinstance(t, int) or t is None else t.data_ptr()
    host._chk(host.lib().ita_mha_long_heads_int8_propagate(eng._h, 0, ptr(x), x.shape[0], x.shape[1] if S is None else S, ptr(w),
                                                           n_w, ptr(out), host._stream_ptr(eng.device)))


@pytest.mark.parametrize("S,R", [(128, 64), (256, 64), (384, 64), (384, 1), (384, 17)])
@pytest.mark.parametrize("H", [2, 3, 4, 6])
@pytest.mark.parametrize("E", [64, 128])
def test_definition(engines, E, H, S, R):
    """one query tile, both ring slots, an odd tile count; R = 64 fills every weight group (two workgroups along z at H = 6),
    R = 17 puts one row in the second group and masks fifteen, R = 1 runs one group with fifteen rows masked"""
    x, w, want = reference(E, H, S)
    for a in range(H):
        for b in range(a + 1, H):
            assert (want[:, a] != want[:, b]).any(), f"heads {a} and {b} alike"
    got = engines(E, H).attention_propagate_long_heads(cu(x), cu(w[:, :R]))
    assert got.dtype == torch.int32 and tuple(got.shape) == (3, H, R, S)
    np.testing.assert_array_equal(got.cpu().numpy(), want[:, :, :R])


@pytest.mark.parametrize("E,H", [(64, 3), (128, 4)])
def test_flat_keys(engines, E, H):
    """test_gpu_long_heads_stats.py's S = 2048 flat-key frame: row sums above 65 280 in every head (asserted there for
    these inputs), so inv_hi reaches 0 and 1 in the row-parameter images"""
    t = case(FIXTURE[E])[4]
    x = long_f32(SEED, 1, 2048, E, t).copy()
    x[:, 128:] = x[:, 600]
    w = lpc.weights(2048, 3)[:1, :17]
    got = engines(E, H).attention_propagate_long_heads(cu(x), cu(w))
    np.testing.assert_array_equal(got.cpu().numpy(), propagate_heads(x, t, w, H))


@pytest.mark.parametrize("E,H", [(64, 6), (128, 2)])
def test_identities(engines, E, H):
    """the ones row is attention_received_long_heads, the minus-ones row its negative, one-hot rows are the probability
    rows of every head"""
    S, eng = 1024, engines(E, H)
    xc = cu(long_f32(SEED, 2, S, E, case(FIXTURE[E])[4]))
    rows = [0, 127, 128, S - 1]
    w = np.zeros((2, 2 + len(rows), S), np.int8)
    w[:, 0], w[:, 1] = 1, -1
    for n, r in enumerate(rows):
        w[:, 2 + n, r] = 1
    got = eng.attention_propagate_long_heads(xc, cu(w))
    received = eng.attention_received_long_heads(xc)
    assert int(received.max()) > 0
    assert torch.equal(got[:, :, 0], received) and torch.equal(got[:, :, 1], -received)
    assert torch.equal(got[:, :, 2:], eng.attention_rows_long_heads(xc, rows).to(torch.int32))


def test_batch_and_repeat(engines):
    """frame b of a B = 3 call is the B = 1 call; a second call gives the same bytes; x is read only"""
    E, H, S, R = 128, 6, 384, 33
    eng = engines(E, H)
    x, w, want = reference(E, H, S)
    xc, wc = cu(x), cu(w[:, :R])
    got = eng.attention_propagate_long_heads(xc, wc)
    for b in range(3):
        assert torch.equal(eng.attention_propagate_long_heads(xc[b:b + 1].contiguous(), wc[b:b + 1].contiguous()), got[b:b + 1]), b
    assert torch.equal(eng.attention_propagate_long_heads(xc, wc), got)
    np.testing.assert_array_equal(got.cpu().numpy(), want[:, :, :R])
    assert torch.equal(xc, cu(x)), "x was written to"


def test_one_head_and_refusals(engines):
    """an H = 1 blob runs the one-head entry (axis inserted); a float blob, seq_len = 200, n_w = 0 and 65, a NULL w and a
    skewed out are refused with out untouched; a correct call still passes afterwards; the one-head entry refuses H > 1"""
    E, S = 64, 256
    e1, e3 = engines(E, 1), engines(E, 3)
    x, w, want = reference(E, 3, S)
    xc, wc = cu(x[:1]), cu(w[:1, :4])
    got = e1.attention_propagate_long_heads(xc, wc)
    assert tuple(got.shape) == (1, 1, 4, S) and torch.equal(got, e1.attention_propagate_long(xc, wc)[:, None])
    np.testing.assert_array_equal(got.cpu().numpy(), propagate_heads(x[:1], case(FIXTURE[E])[4], w[:1, :4], 1))
    c = Canaries({"out": ((1, 3, 4, S), torch.int32)}, pad=32)
    out = c.ptr("out")
    refused(lambda: raw_call(e3, xc, wc, out, 4, S=200), c, UNSUPPORTED)
    ef = host.Engine(params.blob_from_float_params(synth.float_params(1, E=64, num_layers=1, tail=True), 1), device=0)
    refused(lambda: raw_call(ef, xc, wc, out, 4), c, UNSUPPORTED)
    ef.close()
    for n_w in (0, 65):
        refused(lambda: raw_call(e3, xc, wc, out, n_w), c, INVALID)
    refused(lambda: raw_call(e3, xc, None, out, 4), c, INVALID)
    refused(lambda: raw_call(e3, xc, wc, c.ptr("out", 4), 4), c, INVALID)
    with pytest.raises(host.ITAError, match=UNSUPPORTED):
        e3.attention_propagate_long(xc, wc)
    np.testing.assert_array_equal(e3.attention_propagate_long_heads(xc, wc).cpu().numpy(), want[:1, :, :4], err_msg="after the refusals")


def test_captured_call_replays(engines):
    """one eager call (the workspace is held), then the call captured on one stream and replayed twice, with x and w
    rewritten between the replays"""
    E, H, S, B, R = 64, 3, 256, 3, 17
    eng = engines(E, H)
    x, w, want = reference(E, H, S)
    xc, wc = cu(x), cu(w[:, :R])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = eng.attention_propagate_long_heads(xc, wc)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(eager.cpu().numpy(), want[:, :, :R], err_msg="eager")
    c = Canaries({"out": ((B, H, R, S), torch.int32)})
    out = c.views()["out"]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        raw_call(eng, xc, wc, out, R)
    g.replay()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), want[:, :, :R], err_msg="first replay")
    c.assert_untouched(written=("out",))
    order = [2, 0, 1]      # the frames in another order, other weight rows
    xc.copy_(cu(x[order]))
    wc.copy_(cu(w[order, 40:40 + R]))
    c.refill()
    g.replay()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), want[order][:, :, 40:40 + R], err_msg="second replay")
    c.assert_untouched(written=("out",))
    del g


@pytest.mark.parametrize("E", [128, 64])
def test_rollout_equals_the_definition(oracle, E):
    """the two-layer E = 128, H = 4 fixture and the one-layer E = 64, H = 3 fixture as they are"""
    _, H, _, nl, t, fp, fblob = case(FIXTURE[E])
    assert (H, nl) == ((4, 2) if E == 128 else (3, 1))
    S, B = 256, 2
    x = long_f32(SEED, B, S, E, t)
    eng = host.Engine(fblob, device=0)
    xc = cu(x)
    for rows in ((0, 100, 255), None):
        got = eng.attention_rollout_long_heads(xc, rows)
        want = arhr.rollout(oracle, x, t, fp, nl, H, rows)
        assert got.dtype == torch.float64 and tuple(got.shape) == want.shape == (B, 3 if rows else 1, S)
        np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=f"rows={rows}")
    if nl == 2:      # from the second layer on: x enters layer 1
        got = eng.attention_rollout_long_heads(xc, (5, 3), first_layer=1)
        np.testing.assert_array_equal(got.cpu().numpy(), arhr.rollout(oracle, x, t, fp, nl, H, (5, 3), first_layer=1))
    rows = [int(r) for r in np.random.RandomState(7).permutation(S)[:22]]      # two chunks; the same rows one at a time
    many = eng.attention_rollout_long_heads(xc, rows)
    assert tuple(many.shape) == (B, 22, S)
    for n, r in enumerate(rows):
        assert torch.equal(many[:, n:n + 1], eng.attention_rollout_long_heads(xc, [r])), (n, r)
    assert torch.equal(xc, cu(x)), "x was written to"
    eng.close()
