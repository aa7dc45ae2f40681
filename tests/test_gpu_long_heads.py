"""Long-sequence int8 attention with H = 2, 3, 4 or 6 heads on the MI355X (ita_mha_long_heads_q8 / _int8 / _int8_taps,
ita_encoder_layer_long_heads; csrc/ita_long_heads_kernel.h): every output and tap equal to mha_heads_ref.mha.

Weights: the E = 64, H = 3 fixture and layer 0 / 1 of the E = 128, H = 4 two-layer fixture, packed with the head count
under test (nothing but the blob header depends on H).  Inputs: long_cases.long_f32 / long_inputs, seed 5, B = 2.  Every
case asserts from the reference alone that every softmax row of every head is alive and that out_q differs from the
one-head result: a kernel that ignored H, or killed a head, cannot pass."""
import functools

import numpy as np
import pytest
import torch

from drone_oa_iree_vit_accelerator_amd import host, params, synth
from drone_oa_iree_vit_accelerator_amd import mha_heads_ref as ref
from gpu_support import INVALID, UNSUPPORTED, Canaries, cu, engine_pool, refused
from heads_common import FIX_HEADS, FIX_HEADS_2L, case, encoder_layer, heads_of
from long_cases import long_f32

pytestmark = pytest.mark.gpu

SEED, B = 5, 2


def weights(E):
    """(fixture record, num_layers, block tensors, float parameters) of the fixture that gives E its weights"""
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
def reference(E, H, S):
    """(x, out, taps) of mha_heads_ref.mha for the module's inputs; read-only"""
    t = weights(E)[2]
    x = long_f32(SEED, B, S, E, t)
    out, tp = ref.mha(x, t, H)
    assert (tp["probs"].astype(np.int64).sum(-1) > 0).all(), "a head's softmax row is dead in the reference"
    assert (tp["out_q"] != ref.mha(x, t, 1)[1]["out_q"]).mean() > 0.5, "the head count does not show in out_q"
    return x, out, tp


@pytest.mark.parametrize("S", [128, 384])
@pytest.mark.parametrize("H", [2, 3, 4, 6])
@pytest.mark.parametrize("E", [64, 128])
def test_mha_long_heads(engines, E, H, S):
    """one key tile, and an odd tile count (ring-slot parity, the tile-0 prefetch across sweeps); both I/O forms; frame 1
    alone equals frame 1 of the batch"""
    eng = engines(E, H)
    x, out, tp = reference(E, H, S)
    np.testing.assert_array_equal(eng.mha_long_heads_q8(cu(tp["x_q"])).cpu().numpy(), tp["out_q"])
    got = eng.mha_long_heads(cu(x))
    np.testing.assert_array_equal(got.cpu().numpy(), out)
    assert torch.equal(eng.mha_long_heads(cu(x[1:])), got[1:])


@pytest.mark.parametrize("E,H", [(64, 6), (128, 2)])
def test_taps(engines, E, H):
    """the most padded head (two of four lane groups) and the two-step head, S = 256"""
    eng = engines(E, H)
    x, out, tp = reference(E, H, 256)
    rows = [0, 15, 16, 127, 128, 255]
    y, got = eng.mha_long_heads_taps(cu(x), rows)
    got = {k: v.cpu().numpy() for k, v in got.items()}
    for k in ("x_q", "Q", "K", "V", "ctx", "out_q"):
        np.testing.assert_array_equal(got[k], tp[k], err_msg=k)
    logits = tp["logits"][:, :, rows].astype(np.int64)
    np.testing.assert_array_equal(got["logits"], tp["logits"][:, :, rows])
    np.testing.assert_array_equal(got["probs"], tp["probs"][:, :, rows])
    np.testing.assert_array_equal(got["row_max"], logits.max(-1))
    shift = logits.max(-1, keepdims=True) - logits
    np.testing.assert_array_equal(got["row_sum"], np.where(shift > 31, 0, 256 >> np.minimum(shift, 31)).sum(-1))
    assert torch.equal(y, eng.mha_long_heads(cu(x)))
    assert torch.equal(eng.attention_rows_long_heads(cu(x), rows), cu(got["probs"]))


@pytest.mark.parametrize("E,H", [(128, 4), (64, 3)])
def test_layer(oracle, engines, E, H):
    """encoder_layer_long_heads against the composition around mha_heads_ref, every layer, also in place; encode_long_heads
    is the layers chained; at S = 128 the layer is the block kernels' encoder_layer bit for bit"""
    eng = engines(E, H)
    _, nl, t, fp = weights(E)
    x = long_f32(SEED, B, 256, E, t)
    xc, want = cu(x), x
    for l in range(nl):
        want = encoder_layer(oracle, want, t, fp, H, l)[1]
        got = eng.encoder_layer_long_heads(xc, l)
        np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=f"layer {l}")
        alias = xc.clone()
        assert eng.encoder_layer_long_heads(alias, l, out=alias) is alias and torch.equal(alias, got), f"layer {l} in place"
        xc = got
    assert torch.equal(eng.encode_long_heads(cu(x)), xc)
    x128 = cu(x[:, :128])
    for l in range(nl):
        assert torch.equal(eng.encoder_layer_long_heads(x128, l), eng.encoder_layer(x128, l)), f"layer {l} at S = 128"


def test_one_long_case(engines):
    """S = 2048: sixteen key tiles, and row sums above 65 280 in every head, where inv_hi truncates"""
    E, H, S = 128, 4, 2048
    t = weights(E)[2]
    x = long_f32(SEED, 1, S, E, t).copy()
    x[:, 128:] = x[:, 600]        # flat keys: the plain inputs' row sums stay below 3000
    out_q, row_sum = ref.mha_blocked(x, t, H)
    assert (row_sum.max(-1) > 65280).all(), row_sum.max(-1)
    x_q = ref.quantize(x, t["attn0.scal"][ref.INV_SX])
    np.testing.assert_array_equal(engines(E, H).mha_long_heads_q8(cu(x_q)).cpu().numpy(), out_q)


def test_refusals(engines):
    """a float blob, a bad seq_len, too many rows: refused before any launch, outputs untouched; an H = 1 blob runs its
    H = 1 siblings; the handle runs on after a refusal"""
    E, H = 64, 3
    eng = engines(E, H)
    x, out, tp = reference(E, H, 128)
    c = Canaries({"y": ((1, 256, E), torch.float32), "probs": ((1, H, 1025, 256), torch.uint8)})
    into = lambda e, xs, S: host._chk(host.lib().ita_mha_long_heads_int8(e._h, 0, xs.data_ptr(), c.ptr("y"), 1, S, host._stream_ptr(e.device)))
    xs = torch.zeros((1, 256, E), dtype=torch.float32, device="cuda")
    for S in (200, 0):
        refused(lambda: into(eng, xs, S), c, UNSUPPORTED)
    st = host._MhaLongTaps(probs=c.ptr("probs"))
    st.rows, st.n_rows = (host.C.c_int * 1025)(*range(1025)), 1025
    refused(lambda: host._chk(host.lib().ita_mha_long_heads_int8_taps(eng._h, 0, xs.data_ptr(), c.ptr("y"), 1, 256, host.C.byref(st),
                                                                      host._stream_ptr(eng.device))), c, INVALID)
    ef = host.Engine(params.blob_from_float_params(synth.float_params(1, E=64, num_layers=1, tail=True), 1), device=0)
    refused(lambda: into(ef, xs, 256), c, UNSUPPORTED)
    ef.close()
    np.testing.assert_array_equal(eng.mha_long_heads(cu(x)).cpu().numpy(), out)
    e1 = engines(E, 1)
    assert torch.equal(e1.mha_long_heads(cu(x)), e1.mha_long(cu(x)))
    assert torch.equal(e1.mha_long_heads_q8(cu(tp["x_q"])), e1.mha_long_q8(cu(tp["x_q"])))
    assert torch.equal(e1.encoder_layer_long_heads(cu(x)), e1.encoder_layer_long(cu(x)))
