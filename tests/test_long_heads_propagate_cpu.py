"""CPU-side checks of the per-head definitions ita_mha_long_heads_int8_propagate and Engine.attention_rollout_long_heads
are tested against: at H = 1 they are the one-head definitions, and the all-ones row is stats_heads' col_mass."""
import numpy as np

from drone_oa_iree_vit_accelerator_amd import attention_propagate_ref, attention_rollout_heads_ref, attention_rollout_ref
from drone_oa_iree_vit_accelerator_amd.attention_propagate_heads_ref import propagate_heads
from drone_oa_iree_vit_accelerator_amd.attention_stats_heads_ref import stats_heads
from heads_common import FIX_HEADS, FIX_HEADS_2L, case, heads_of
from long_cases import long_f32
from long_propagate_common import weights

T = case([p for p in FIX_HEADS if heads_of(p) == 3][0])[4]     # E = 64 block tensors


def test_one_head_is_propagate_ref():
    """two query blocks of 128 against one of 256"""
    x, w = long_f32(5, 3, 256, 64, T), weights(256, 3)[:, :17]
    got = propagate_heads(x, T, w, 1, block=128)
    assert got.dtype == np.int32
    np.testing.assert_array_equal(got, attention_propagate_ref.propagate(x, T, w)[:, None])


def test_ones_row_is_col_mass():
    H = 3
    x = long_f32(5, 2, 256, 64, T)
    got = propagate_heads(x, T, np.ones((1, 256), np.int8), H)
    np.testing.assert_array_equal(got[:, :, 0], stats_heads(x, T, H)["col_mass"])
    assert (got[:, 0] != got[:, 1]).any(), "the head count does not show"


def test_one_head_rollout_is_rollout_ref(oracle):
    """two layers (the E = 128 fixture's tensors, read with one head), from layer 0 and from layer 1"""
    _, _, E, nl, t, fp, _ = case(FIX_HEADS_2L[0])
    x = long_f32(5, 1, 128, E, t)
    for first in (0, 1):
        np.testing.assert_array_equal(attention_rollout_heads_ref.rollout(oracle, x, t, fp, nl, 1, (0, 77), first),
                                      attention_rollout_ref.rollout(oracle, x, t, fp, nl, (0, 77), first))
