"""CPU-side checks of the per-head long-sequence statistics' definition (attention_stats_heads_ref.stats_heads, what
ita_mha_long_heads_int8_stats is tested against): at H = 1 it is attention_stats_ref.stats, at H > 1 each head's
statistics are the sums of the probabilities mha_heads_ref.mha taps."""
import numpy as np

from drone_oa_iree_vit_accelerator_amd import attention_stats_ref
from drone_oa_iree_vit_accelerator_amd import mha_heads_ref as ref
from drone_oa_iree_vit_accelerator_amd.attention_stats_heads_ref import stats_heads
from heads_common import FIX_HEADS, case, heads_of
from long_cases import long_f32

T = case([p for p in FIX_HEADS if heads_of(p) == 3][0])[4]     # E = 64 block tensors


def test_one_head_is_stats_ref():
    """two query blocks of 128 against one of 256"""
    x = long_f32(5, 2, 256, 64, T)
    want, got = attention_stats_ref.stats(x, T), stats_heads(x, T, 1, block=128)
    for k in attention_stats_ref.NAMES:
        assert got[k].dtype == want[k].dtype
        np.testing.assert_array_equal(got[k], want[k][:, None], err_msg=k)


def test_heads_are_the_sums_of_the_tapped_probabilities():
    H = 3
    x = long_f32(5, 2, 128, 64, T)
    tp = ref.mha(x, T, H)[1]
    p = tp["probs"].astype(np.int64)                            # (B, H, 128, 128)
    assert p.shape == (2, H, 128, 128) and (p.sum(-1) > 0).all()
    got = stats_heads(x, T, H)
    np.testing.assert_array_equal(got["row_max"], tp["logits"].max(-1))
    for k, want in (("row_mass", p.sum(-1)), ("row_nnz", (p > 0).sum(-1)), ("col_mass", p.sum(-2)), ("col_nnz", (p > 0).sum(-2))):
        np.testing.assert_array_equal(got[k], want, err_msg=k)
    assert (got["col_mass"] != stats_heads(x, T, 1)["col_mass"]).any(), "the head count does not show"
