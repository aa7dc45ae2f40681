"""Long float propagation at the long end on the MI355X: ita_mha_long_f32_propagate at S = 8192 and S = 65536, one frame.

S = 8192, R = 16: all ones, uniform, signed normal, a one-hot at the last query and twelve more signed rows, against float64
with the whole 8192 x 8192 matrix formed 1024 query rows at a time (long_limits_common.rows64) and the project's bound
3 e_torch + 4 ulp32(max |truth|), e_torch from torch's CPU f32 evaluation in the same chunks (rows32).  S = 65536: a frame
drawn from 192 distinct tokens, 64 of them single (long_limits_common.vocab_f32_frame) and weights that are constant on
every class of equal tokens, so that out = (c * counts) @ P[representatives] follows from 192 rows of the matrix in float64
and in torch f32; the one-hot at the last query (a single) is such a weight row.  The one-hot rows have the taps' bits.

Error / bound measured on the MI355X: 0.09 (plain, E = 64) and 0.10 (ramp, E = 128) at S = 8192; 0.22 (E = 64) and 0.26
(E = 128) at S = 65536."""
import functools

import numpy as np
import pytest

from drone_oa_iree_vit_accelerator_amd import host
from gpu_support import cu
import long_f32_common as lc
import long_f32_taps_common as ltc
import long_limits_common as ll

pytestmark = pytest.mark.gpu

VOCAB = (192, 64, 3)                # V, singles, seed: the float statistics' vocabulary frames
R = 16


def _bound(t, r):
    e = float(np.abs(r - t).max())
    return 3.0 * e + 4.0 * ltc.ulp32(np.abs(t).max()), e


def _weights(S, seed, hot):
    rs = np.random.RandomState(seed)
    w = rs.standard_normal((1, R, S)).astype(np.float32)
    w[0, 0] = 1.0
    w[0, 1] = rs.random_sample(S).astype(np.float32)
    w[0, 3] = 0.0
    w[0, 3, hot] = 1.0
    return w


@functools.lru_cache(maxsize=None)
def _ref_8192(kind, E, chunk=1024):
    """(w, float64 out, bound, e_torch) of one frame lc.inputs(kind, E, 8192, 1)"""
    import torch
    S = 8192
    fp, _, twin = lc.case(E)
    x, w = lc.inputs(kind, E, S, 1), _weights(S, 11, S - 1)
    t, r = np.zeros((1, R, S)), torch.zeros((1, R, S), dtype=torch.float32)
    for r0 in range(0, S, chunk):
        rows = range(r0, min(r0 + chunk, S))
        t += w[:, :, r0:r0 + chunk].astype(np.float64) @ ll.rows64(x, fp, 0, rows, tail=False)["probs"]
        r += torch.matmul(torch.from_numpy(w[:, :, r0:r0 + chunk].copy()), torch.from_numpy(ll.rows32(x, twin, 0, rows, tail=False)["probs"]))
    return (w, t) + _bound(t, r.numpy())


@pytest.mark.parametrize("kind,E", [("plain", 64), ("ramp", 128)])
def test_propagate_at_8192_against_float64(kind, E):
    import torch
    S = 8192
    w, t, bound, e = _ref_8192(kind, E)
    eng = host.Engine(lc.case(E)[1], device=0)
    x = cu(lc.inputs(kind, E, S, 1))
    got = eng.attention_propagate_long_f32(x, cu(w))
    g = got.cpu().numpy()
    err = float(np.abs(g - t).max())
    print(f"propagate {kind} E={E} S={S}: |gpu - float64| = {err:.3e}, e_torch {e:.3e}, bound {bound:.3e}, err / bound {err / bound:.2f}")
    assert np.isfinite(g).all() and err <= bound
    assert torch.equal(got[:, 3].view(torch.int32), eng.attention_rows_long_f32(x, [S - 1])[:, 0].view(torch.int32)), "the one-hot row"
    assert float(got[:, 0].sum(dtype=torch.float64)) == pytest.approx(S, rel=1e-5)
    eng.close()


@functools.lru_cache(maxsize=None)
def _ref_65536(E):
    """(w, float64 out, bound, e_torch) of the vocabulary frame in the class form"""
    S = 65536
    V, singles, seed = VOCAB
    fp, _, twin = lc.case(E)
    x = ll.vocab_f32_frame(E, S, V, singles, seed)
    _, reps, cls, counts = ll.vocabulary(S, V, singles, seed)
    rs = np.random.RandomState(5)
    c = rs.standard_normal((R, V)).astype(np.float32)        # a weight per row and class
    c[0] = 1.0
    c[1] = rs.random_sample(V).astype(np.float32)
    c[3] = 0.0
    c[3, cls[S - 1]] = 1.0                                    # the last query is a single: a one-hot row
    assert counts[cls[S - 1]] == 1
    w = np.ascontiguousarray(c[:, cls][None])
    p64 = ll.rows64(x, fp, 0, reps, tail=False)["probs"]
    p32 = ll.rows32(x, twin, 0, reps, tail=False)["probs"]
    t = (c.astype(np.float64) * counts.astype(np.float64)[None])[None] @ p64
    r = (c * counts.astype(np.float32)[None])[None] @ p32
    assert r.dtype == np.float32
    return (w, t) + _bound(t, r)


@pytest.mark.parametrize("E", [64, 128])
def test_propagate_at_65536_on_a_vocabulary_frame(E):
    import torch
    S = 65536
    V, singles, seed = VOCAB
    w, t, bound, e = _ref_65536(E)
    eng = host.Engine(lc.case(E)[1], device=0)
    x = cu(ll.vocab_f32_frame(E, S, V, singles, seed))
    got = eng.attention_propagate_long_f32(x, cu(w))
    g = got.cpu().numpy()
    err = float(np.abs(g - t).max())
    print(f"propagate vocabulary E={E} S={S}: |gpu - float64| = {err:.3e}, e_torch {e:.3e}, bound {bound:.3e}, err / bound {err / bound:.2f}")
    assert np.isfinite(g).all() and err <= bound
    assert torch.equal(got[:, 3].view(torch.int32), eng.attention_rows_long_f32(x, [S - 1])[:, 0].view(torch.int32)), "the one-hot row"
    assert torch.equal(got.view(torch.int32), eng.attention_propagate_long_f32(x, cu(w)).view(torch.int32))
    eng.close()
