"""Long int8 attention on ragged batches on the MI355X (ita_mha_long_int8_ragged, ita_encoder_layer_long_ragged;
csrc/ita_long_ragged_kernel.h): rows below a frame's length equal the one-head definition on the unpadded frame bit for
bit, whatever the padding holds.  Cases, inputs (padding: 4 x noise) and definition: ragged_cases.py."""
import numpy as np
import pytest
import torch

from drone_oa_iree_vit_accelerator_amd import host, params, synth
from gpu_support import INVALID, UNSUPPORTED, Canaries, cu, engine_pool, refused, same_bits
from heads_common import FIX_HEADS, case as heads_case, encoder_layer, heads_of
from long_cases import long_case
from ragged_cases import CASES, case_id, definition, inputs, weights

pytestmark = pytest.mark.gpu

lens_t = lambda lens: torch.tensor(lens, dtype=torch.int32, device="cuda")


@pytest.fixture(scope="module")
def engines():
    yield from engine_pool(lambda E: weights(E).blob)


@pytest.mark.parametrize("case", CASES, ids=case_id)
@pytest.mark.parametrize("E", [64, 128])
def test_definition(engines, E, case):
    """valid rows: mha_heads_ref.mha of the unpadded frame; rows past the length: 0"""
    got = engines(E).mha_long_ragged(cu(inputs(E, *case)), lens_t(case[1]))
    np.testing.assert_array_equal(got.cpu().numpy(), definition(E, *case))


@pytest.mark.parametrize("S_pad", [256, 1024])
@pytest.mark.parametrize("E", [64, 128])
def test_full_lengths(engines, E, S_pad):
    """lens == S_pad (and above: clamped) is mha_long"""
    x = cu(inputs(E, S_pad, (S_pad, S_pad)))
    assert torch.equal(engines(E).mha_long_ragged(x, lens_t((S_pad, S_pad + 5))), engines(E).mha_long(x))


@pytest.mark.parametrize("E", [64, 128])
def test_poisoned_padding(engines, E):
    """NaN and +-Inf behind the valid tokens change nothing"""
    S_pad, lens = 256, (200,)
    x = inputs(E, S_pad, lens).copy()
    x[:, 200:] = np.resize(np.array([np.nan, np.inf, -np.inf], np.float32), x[:, 200:].shape)
    np.testing.assert_array_equal(engines(E).mha_long_ragged(cu(x), lens_t(lens)).cpu().numpy(), definition(E, S_pad, lens))


@pytest.mark.parametrize("case", [CASES[-1], CASES[4]], ids=case_id)
@pytest.mark.parametrize("E", [64, 128])
def test_layer(oracle, engines, E, case):
    """encoder_layer_long_ragged, every layer, against the composition around mha_heads_ref on the unpadded frames; padded
    rows finite; out aliasing x; encode_long_ragged is the layers chained"""
    eng, w, (S_pad, lens) = engines(E), weights(E), case
    x, lt = inputs(E, S_pad, lens), lens_t(lens)
    xc, want = cu(x), [x[b:b + 1, :n] for b, n in enumerate(lens)]
    for l in range(w.num_layers):
        got = eng.encoder_layer_long_ragged(xc, lt, l)
        assert bool(torch.isfinite(got).all()), f"layer {l}"
        for b, n in enumerate(lens):
            if n:
                want[b] = encoder_layer(oracle, want[b], w.t, w.fp, 1, l)[1]
                np.testing.assert_array_equal(got[b, :n].cpu().numpy(), want[b][0], err_msg=f"layer {l} frame {b}")
        alias = xc.clone()
        assert eng.encoder_layer_long_ragged(alias, lt, l, out=alias) is alias and torch.equal(alias, got), f"layer {l} in place"
        xc = got
    assert torch.equal(eng.encode_long_ragged(cu(x), lt), xc)


@pytest.mark.parametrize("E", [64, 128])
def test_in_place_and_repeat(engines, E):
    S_pad, lens = CASES[-1]
    x, lt = cu(inputs(E, S_pad, lens)), lens_t(lens)
    first = engines(E).mha_long_ragged(x, lt)
    assert torch.equal(engines(E).mha_long_ragged(x, lt), first)
    host._chk(host.lib().ita_mha_long_int8_ragged(engines(E)._h, 0, x.data_ptr(), x.data_ptr(), len(lens), S_pad, lt.data_ptr(),
                                                  host._stream_ptr(0)))
    assert torch.equal(x, first)


@pytest.mark.parametrize("E", [64, 128])
def test_capture_follows_new_lengths(engines, E):
    """one captured call (gpu_support's protocol: a call before the capture, several replays against the eager result,
    canaries behind the output) follows the lengths that lie in device memory at each replay"""
    eng, (S_pad, lens) = engines(E), CASES[-1]
    x, lt = cu(inputs(E, S_pad, lens)), lens_t(lens)
    c = Canaries({"y": (tuple(x.shape), torch.float32)})
    eng.mha_long_ragged(x, lt)      # the workspace has its size before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        host._chk(host.lib().ita_mha_long_int8_ragged(eng._h, 0, x.data_ptr(), c.ptr("y"), len(lens), S_pad, lt.data_ptr(),
                                                      host._stream_ptr(0)))
    for replay, now in enumerate((lens, lens, (5, 384, 130, 256, 0), lens)):
        lt.copy_(lens_t(now))
        g.replay()
        torch.cuda.synchronize()
        assert same_bits(c.views(), {"y": eng.mha_long_ragged(x, lens_t(now))}, ("y",)), (replay, now)
        c.assert_untouched(written=("y",))
        c.refill()
    del g


def test_refusals(engines):
    """refused before any launch, outputs untouched; the handle runs on"""
    E, S_pad, lens = 64, 256, (200,)
    x, lt = cu(inputs(E, S_pad, lens)), lens_t(lens)
    c = Canaries({"y": ((1, S_pad, E), torch.float32)})
    L = host.lib()
    mha = lambda e, S=S_pad, lp=lt.data_ptr(): host._chk(L.ita_mha_long_int8_ragged(e._h, 0, x.data_ptr(), c.ptr("y"), 1, S, lp, host._stream_ptr(0)))
    layer = lambda e, S=S_pad, lp=lt.data_ptr(): host._chk(L.ita_encoder_layer_long_ragged(e._h, 0, x.data_ptr(), c.ptr("y"), 1, S, lp, host._stream_ptr(0)))
    blobs = {"H = 3": heads_case([p for p in FIX_HEADS if heads_of(p) == 3][0])[6],
             "ITAW0003": params.blob_from_float_params(synth.float_params(1, E=64, num_layers=1, tail=True), 1)}
    for blob in blobs.values():
        e = host.Engine(blob, device=0)
        for entry in (mha, layer):
            refused(lambda: entry(e), c, UNSUPPORTED)
        e.close()
    e2 = host.Engine(long_case("onlyattn1l_E64_s0_B2").blob, device=0)     # ITAW0002: int8 attention, float FFN
    refused(lambda: layer(e2), c, UNSUPPORTED)
    e2.close()
    eng = engines(E)
    for entry in (mha, layer):
        for S in (200, 0):
            refused(lambda: entry(eng, S=S), c, UNSUPPORTED)
        for lp in (None, lt.data_ptr() + 2):
            refused(lambda: entry(eng, lp=lp), c, INVALID)
    for bad in (lt.long(), lens_t((200, 200)), lt.cpu()):
        for call in (eng.mha_long_ragged, eng.encoder_layer_long_ragged, eng.encode_long_ragged):
            with pytest.raises(host.ITAError, match="lens must be"):
                call(x, bad)
    np.testing.assert_array_equal(eng.mha_long_ragged(x, lt).cpu().numpy(), definition(E, S_pad, lens))
