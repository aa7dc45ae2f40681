"""Per-head long-sequence attention statistics on the MI355X: ita_mha_long_heads_int8_stats
(Engine.attention_stats_long_heads / attention_received_long_heads; csrc/ita_long_heads_stats_kernel.h), every array equal
to attention_stats_heads_ref.stats_heads.  The path is integer: every comparison is assert_array_equal.

Weights and inputs are test_gpu_long_heads.py's: the E = 64, H = 3 fixture and layer 0 of the E = 128, H = 4 two-layer
fixture, packed with the head count under test; long_cases.long_f32, seed 5.  As there, the E = 64 fixture selects the FAST
(single-rounding) instantiations of the kernel and the E = 128 fixture the exact ones."""
import functools

import numpy as np
import pytest
import torch

from drone_oa_iree_vit_accelerator_amd import host, params, synth
from drone_oa_iree_vit_accelerator_amd.attention_stats_heads_ref import stats_heads
from drone_oa_iree_vit_accelerator_amd.attention_stats_ref import NAMES
from gpu_support import UNSUPPORTED, Canaries, cu, engine_pool, refused, to_numpy
from heads_common import FIX_HEADS, FIX_HEADS_2L, case, heads_of
from long_cases import long_f32

pytestmark = pytest.mark.gpu

SEED = 5


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
def reference(E, H, S, B=2):
    """(x, stats_heads of it) for the module's inputs; read-only"""
    t = weights(E)[2]
    x = long_f32(SEED, B, S, E, t)
    return x, stats_heads(x, t, H)


def equal(got, want, names=NAMES):
    got = to_numpy(got)
    for k in names:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


@pytest.mark.parametrize("S", [128, 256, 384])
@pytest.mark.parametrize("H", [2, 3, 4, 6])
@pytest.mark.parametrize("E", [64, 128])
def test_stats(engines, E, H, S):
    """one, two and three key tiles: the ring wrapping between sweeps, both parities of the column table and its last flush
    after an odd and an even tile count"""
    x, want = reference(E, H, S)
    assert (want["row_mass"] > 0).all() and (want["col_mass"][:, 0] != want["col_mass"][:, 1]).any(), "dead rows, or heads alike"
    equal(engines(E, H).attention_stats_long_heads(cu(x)), want)


@pytest.mark.parametrize("E,H", [(64, 3), (128, 4)])
def test_flat_keys(engines, E, H):
    """test_gpu_long_heads.py's S = 2048 flat-key frame: row sums above 65 280 in every head, many keys per row alive, so
    row_nnz and col_nnz are far from 0 and 1 and the 16-bit halves of the column table carry real load.  The stock frame
    meets the two conditions below unscaled (row_nnz up to 44 and 20, 65 and 46 distinct col_nnz); at E = 64 head 4 of 6
    stays below 65 280, hence H = 3 there."""
    t = weights(E)[2]
    x = long_f32(SEED, 1, 2048, E, t).copy()
    x[:, 128:] = x[:, 600]
    want = stats_heads(x, t, H)
    assert (want["row_sum"].max(-1) > 65280).all(), want["row_sum"].max(-1)
    assert want["row_nnz"].max() > 16 and len(np.unique(want["col_nnz"])) >= 3, (want["row_nnz"].max(), np.unique(want["col_nnz"]))
    equal(engines(E, H).attention_stats_long_heads(cu(x)), want)


def test_columns_only(engines):
    """the columns-only call gives the full call's col_mass and writes nothing beside its (B, H, S) buffer"""
    E, H, S = 64, 3, 256
    eng = engines(E, H)
    x, want = reference(E, H, S)
    xc = cu(x)
    np.testing.assert_array_equal(eng.attention_received_long_heads(xc).cpu().numpy(), want["col_mass"])
    c = Canaries({"col_mass": ((2, H, S), torch.int32), "row_mass": ((2, H, S), torch.int32)})
    st = host._MhaLongStats(col_mass=c.ptr("col_mass"))
    host._chk(host.lib().ita_mha_long_heads_int8_stats(eng._h, 0, xc.data_ptr(), 2, S, host.C.byref(st), host._stream_ptr(eng.device)))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(c.views()["col_mass"].cpu().numpy(), want["col_mass"])
    c.assert_untouched(written=("col_mass",))


def test_repeat_and_batch(engines):
    """the entry zeroes the column arrays: a second call gives the same bytes; frame b of a B = 3 call is the B = 1 call"""
    E, H, S = 128, 6, 384
    eng = engines(E, H)
    x, want = reference(E, H, S, 3)
    first = eng.attention_stats_long_heads(cu(x))
    equal(eng.attention_stats_long_heads(cu(x)), to_numpy(first))
    equal(first, want)
    for b in range(3):
        equal(eng.attention_stats_long_heads(cu(x[b:b + 1])), {k: v[b:b + 1] for k, v in want.items()})


def test_one_head_and_refusals(engines):
    """an H = 1 blob runs the one-head entry (axis inserted); a float blob and S = 200 are refused, outputs untouched; the
    one-head entry still refuses H > 1"""
    E, S = 64, 256
    e1, e3 = engines(E, 1), engines(E, 3)
    x, want = reference(E, 1, S)
    got = e1.attention_stats_long_heads(cu(x))
    equal(got, want)
    equal({k: v[:, None] for k, v in e1.attention_stats_long(cu(x)).items()}, to_numpy(got))
    c = Canaries({k: ((2, 3, S), torch.int8 if k == "row_max" else torch.int32) for k in NAMES})
    st = host._MhaLongStats(**c.ptrs())
    into = lambda e, seq: host._chk(host.lib().ita_mha_long_heads_int8_stats(e._h, 0, cu(x).data_ptr(), 2, seq, host.C.byref(st),
                                                                             host._stream_ptr(e.device)))
    refused(lambda: into(e3, 200), c, UNSUPPORTED)
    ef = host.Engine(params.blob_from_float_params(synth.float_params(1, E=64, num_layers=1, tail=True), 1), device=0)
    refused(lambda: into(ef, S), c, UNSUPPORTED)
    ef.close()
    with pytest.raises(host.ITAError, match=UNSUPPORTED):
        e3.attention_stats_long(cu(x))
    equal(e3.attention_stats_long_heads(cu(x)), reference(E, 3, S)[1])
