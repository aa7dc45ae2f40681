"""The long float taps on the CPU: an f32 numpy emulation of the two launches of csrc/ita_long_f32_kernel.h
(long_f32_taps_common.emulate: block-summed projections and logits, 64-key units, running m and l, four lane shares added
at the end, ita_expf through the oracle) must meet every bound the GPU test holds the taps to, and six wrong kernels must
land beyond twice the bound -- so the bounds are met by the arithmetic the kernels are meant to run, and are tight enough
to tell a wrong row maximum, row sum, key order or feature order from the right one.  No GPU."""
import numpy as np
import pytest

import long_f32_common as lc
import long_f32_taps_common as ltc

SHAPES = [(128, 2), (384, 2)]
CHECKED = ltc.TENSORS + ("logits", "probs", "row_sum")


@pytest.mark.parametrize("S,B", SHAPES)
@pytest.mark.parametrize("E", [64, 128])
@pytest.mark.parametrize("kind", lc.KINDS)
def test_emulation_meets_every_bound(kind, E, S, B):
    rows = ltc.rows_for(kind, E, S, B)
    got = ltc.emulate(kind, E, S, B, 0, rows)
    bnd, err = ltc.bounds(kind, E, S, B, 0, rows), ltc.errors(got, kind, E, S, B, 0, rows)
    for k in CHECKED:
        print(f"{kind} E={E} S={S} B={B} {k}: err {err[k]:.3e}, e_torch {bnd[k][1]:.3e}, bound {bnd[k][0]:.3e}, err / bound {err[k] / bnd[k][0]:.2f}")
    for k in CHECKED:
        assert err[k] <= bnd[k][0], (k, err[k], bnd[k])
    np.testing.assert_array_equal(got["row_max"], got["logits"].max(-1))


# mutation -> (input kind, the tap that must be beyond twice its bound)
MUTATIONS = {"max_at_unit": ("ramp", "probs"), "lane_missing": ("plain", "row_sum"), "no_rescale": ("ramp", "row_sum"),
             "unit_swapped": ("plain", "logits"), "one_lane_sum": ("plain", "probs"), "one_chain": ("plain", "K")}


@pytest.mark.parametrize("mutation", list(MUTATIONS))
def test_wrong_kernels_are_told_apart(mutation):
    kind, tap = MUTATIONS[mutation]
    E, S, B = 64, 384, 2
    rows = ltc.rows_for(kind, E, S, B)
    got = ltc.emulate(kind, E, S, B, 0, rows, mutation=mutation)
    bnd, err = ltc.bounds(kind, E, S, B, 0, rows), ltc.errors(got, kind, E, S, B, 0, rows)
    print(f"{mutation}: {tap} err {err[tap]:.3e}, bound {bnd[tap][0]:.3e}, err / bound {err[tap] / bnd[tap][0]:.1f}")
    assert err[tap] > 2.0 * bnd[tap][0], (mutation, tap, err[tap], bnd[tap])
