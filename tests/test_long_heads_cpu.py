"""mha_heads_ref.mha_blocked, the head-by-head evaluation in query blocks that test_gpu_long_heads.py compares an
S = 2048 frame against, is mha itself: out_q and the softmax row sums at S = 256, E = 128, H = 4, blocks of 96 rows (a
ragged last block)."""
import numpy as np

from drone_oa_iree_vit_accelerator_amd import mha_heads_ref as ref
from heads_common import FIX_HEADS_2L, case
from long_cases import long_f32


def test_blocked_evaluation_is_mha():
    _, _, E, _, t, _, _ = case(FIX_HEADS_2L[0])
    x = long_f32(5, 2, 256, E, t)
    out_q, row_sum = ref.mha_blocked(x, t, 4, block=96)
    _, tp = ref.mha(x, t, 4)
    np.testing.assert_array_equal(out_q, tp["out_q"])
    logits = tp["logits"].astype(np.int64)
    shift = logits.max(-1, keepdims=True) - logits
    np.testing.assert_array_equal(row_sum, np.where(shift > 31, 0, 256 >> np.minimum(shift, 31)).sum(-1))
