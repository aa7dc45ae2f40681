"""attention_hist_heads_ref: attention_hist_ref.hist with a head axis at H = 1; the class form equals hist_heads on a frame"""
import numpy as np
import pytest

from drone_oa_iree_vit_accelerator_amd import attention_hist_ref as ahr
from drone_oa_iree_vit_accelerator_amd.attention_hist_heads_ref import NAMES, hist_heads, hist_heads_from_classes
from heads_common import FIX_HEADS, FIX_HEADS_2L, case, heads_of
from long_cases import long_f32

T64, T128 = case([p for p in FIX_HEADS if heads_of(p) == 3][0])[4], case(FIX_HEADS_2L[0])[4]


def equal(got, want):
    assert tuple(got) == NAMES
    for k in NAMES:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


@pytest.mark.parametrize("E,t", [(64, T64), (128, T128)])
def test_one_head_is_the_one_head_definition(E, t):
    x = long_f32(5, 2, 256, E, t)
    equal(hist_heads(x, t, 1, block=96), {k: v[:, None] for k, v in ahr.hist(x, t).items()})


@pytest.mark.parametrize("E,t,H", [(64, T64, 6), (128, T128, 2), (128, T128, 3)])
def test_class_form(E, t, H):
    """24 distinct tokens with counts 1 .. 40 in a shuffled frame of 384 positions"""
    rs = np.random.RandomState(3)
    reps = long_f32(5, 1, 32, E, t)[0, :24]
    counts = rs.permutation(np.r_[40, 1, np.full(22, 0)] + np.r_[0, 0, rs.multinomial(343 - 22, np.ones(22) / 22) + 1])
    assert counts.sum() == 384 and counts.min() >= 1
    x = reps[rs.permutation(np.repeat(np.arange(24), counts))][None]
    want = hist_heads(x, t, H)
    assert all(int(want[k][0, h].sum()) == 384 * 384 for k in ("logits", "shifts", "probs") for h in range(H))
    equal(hist_heads_from_classes(reps, counts, t, H), want)
