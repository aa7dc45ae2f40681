"""CPU-side checks of the long float propagation (ita_mha_long_f32_propagate, Engine.attention_propagate_long_f32 /
attention_rollout_long_f32): the f32 numpy model of the kernel's written-down addition order
(long_f32_propagate_common.blocked) stays inside both bounds of the GPU test on every case of that test, its one-hot rows
are bit-exact, six wrong kernels land outside a bound, the float64 definitions agree with dense products, and the entry
refuses bad arguments before it touches the device.  No compute call is made here.

Error / bound of the model over all cases: against its own probabilities (gamma_(S+2) sum |w| p) 0.002 (S = 2048) to 0.036
(flat, E = 128, S = 256); against float64 (3 e_torch + 4 ulp) 0.08 to 0.20 (ramp, E = 64, S = 256)."""
import ctypes

import numpy as np
import pytest

from drone_oa_iree_vit_accelerator_amd import attention_propagate_f32_ref as apr
from drone_oa_iree_vit_accelerator_amd import attention_rollout_f32_ref as arr
from drone_oa_iree_vit_accelerator_amd import attention_rollout_ref
from drone_oa_iree_vit_accelerator_amd import host
import long_f32_common as lc
import long_f32_propagate_common as pc
import long_f32_taps_common as ltc


@pytest.mark.parametrize("E", [64, 128])
@pytest.mark.parametrize("kind,S,B", pc.CASES)
def test_model_of_the_kernel_stays_inside_both_bounds(kind, S, B, E):
    got = pc.modelled(kind, E, S, B)
    assert got.shape == (B, 64, S) and got.dtype == np.float32
    bad, rt, r64 = pc.verdict(got, kind, E, S, B)
    print(f"{kind} E={E} S={S} B={B}: worst error / gamma bound {rt:.4f}, worst error / float64 bound {r64:.4f} "
          f"(bound, e_torch) {pc.refs64(kind, E, S, B)[1:]}")
    assert bad == []                       # includes: one-hot rows have p's bits, the zero row is +0.0
    # the all-ones row is the statistics' col_mass up to the order of the additions
    import long_f32_stats_common as lss
    cm = lss.emulated(kind, E, S, B)[1]["col_mass"].astype(np.float64)
    for r in pc.rows_of("ones"):
        assert (np.abs(got[:, r] - cm) <= 2 * apr.gamma(S) * cm).all()


def test_a_row_does_not_depend_on_its_place():
    """row 37 of the R = 64 model equals the same weights as row 0 of an R = 1 model: rows are independent chains"""
    kind, E, S, B = "ramp", 64, 256, 2
    p = pc.model_probs(kind, E, S, B)[3]
    w = pc.weights(S, B)
    np.testing.assert_array_equal(pc.blocked(w[:, 37:38], p).view(np.int32), pc.modelled(kind, E, S, B)[:, 37:38].view(np.int32))


@pytest.mark.parametrize("mutation", pc.MUTATIONS)
def test_bounds_reject_a_wrong_kernel(mutation):
    """every mutation lands outside at least one bound on at least one committed case"""
    caught = []
    for kind, E, S, B in (("ramp", 64, 256, 2), ("plain", 128, 384, 2)):
        bad, _, _ = pc.verdict(pc.model(kind, E, S, B, mutation=mutation), kind, E, S, B)
        if bad:
            caught.append((kind, E, S, B, bad[0]))
    print(mutation, caught)
    assert caught, mutation


@pytest.mark.parametrize("E", [64, 128])
def test_propagate64_against_dense_product(E):
    S, B = 256, 2
    fp, _ = pc.case("plain", E)
    x, w = pc.inputs("plain", E, S, B), pc.weights(S, B)
    P = ltc.refs("plain", E, S, B)[0]["probs"]
    want = w.astype(np.float64) @ P
    for block in (64, 100, 1024):
        np.testing.assert_allclose(apr.propagate64(x, fp, w, 0, block), want, rtol=1e-11, atol=1e-14)
    np.testing.assert_allclose(apr.propagate64(x, fp, w[0], 0, 128)[1], w[0].astype(np.float64) @ P[1], rtol=1e-11, atol=1e-14)
    p32 = P.astype(np.float32)
    ref, mass = apr.propagate_from_taps(p32, w)
    np.testing.assert_array_equal(ref, w.astype(np.float64) @ p32.astype(np.float64))
    np.testing.assert_array_equal(mass, np.abs(w).astype(np.float64) @ p32.astype(np.float64))
    assert apr.gamma(258) == 258 * 2.0 ** -24 / (1 - 258 * 2.0 ** -24)
    with pytest.raises(ValueError):
        apr.propagate64(x, fp, w[:, :, :128], 0)


def test_rollout64_against_dense_product():
    """the recurrence against the dense float64 product of 0.5 (I + P_l), two layers, S = 128"""
    E, S, B = 128, 128, 2
    fp, _, _ = lc.case(E)
    x0 = lc.inputs("plain", E, S, B)
    xs = [x0.astype(np.float64), lc.layer64(x0, fp, 0)]
    A = [0.5 * (np.eye(S)[None] + apr.probs64(xs[l], fp, l, 0, S)) for l in range(2)]
    rows = [5, 127, 0]
    got = arr.rollout64(xs, fp, rows, 0)
    want = (A[1] @ A[0])[:, rows]
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(arr.rollout64(xs[1:], fp, rows, 1), A[1][:, rows], rtol=1e-12, atol=1e-15)
    u = arr.rollout64(xs, fp, None, 0)
    assert u.shape == (B, 1, S)
    np.testing.assert_allclose(u[:, 0], (A[1] @ A[0]).mean(1), rtol=1e-12)
    np.testing.assert_allclose(got.sum(-1), 1.0, rtol=1e-12)
    assert (got >= 0).all()
    for r in (None, rows):
        np.testing.assert_array_equal(arr.start(B, S, r), attention_rollout_ref.start(B, S, r))


def test_definitions_import_neither_torch_nor_the_oracle():
    import os
    for mod in (apr, arr):
        src = open(mod.__file__).read()
        assert "import torch" not in src and "oracle" not in src, os.path.basename(mod.__file__)


def test_entry_refuses_bad_arguments_without_a_gpu():
    """a null handle is refused before anything is touched (a call with a live handle would go on to the device)"""
    host.build_extension()
    L = host.lib()
    x, w, out = (ctypes.create_string_buffer(64) for _ in range(3))
    assert L.ita_mha_long_f32_propagate(None, 0, ctypes.addressof(x), 1, 128, ctypes.addressof(w), 1, ctypes.addressof(out), None) == -1
    assert L.ita_last_error() == -1 and L.ita_error_string()
    assert not any(out.raw)
