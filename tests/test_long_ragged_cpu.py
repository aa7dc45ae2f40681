"""A condition on the ragged tests' INPUTS, not a second implementation: with the padding ragged_cases.inputs gives, the
definition on the padded frame differs from the definition on the unpadded one in a valid row, for every frame shorter
than S_pad -- so a kernel that forgot the mask cannot pass test_gpu_long_ragged.py.  Skipped, and named here: the empty
frame (frame 3 of the mixed batch), which has no valid row; the frames of one token are held to the condition."""
import pytest

from drone_oa_iree_vit_accelerator_amd import mha_heads_ref as ref
from ragged_cases import CASES, case_id, definition, inputs, weights

SKIPPED_LENS = (0,)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_unmasked_padding_changes_valid_rows(case):
    E, (S_pad, lens) = 64, case
    x, want = inputs(E, S_pad, lens), definition(E, S_pad, lens)
    for b, n in enumerate(lens):
        if n == S_pad or n in SKIPPED_LENS:
            continue
        padded = ref.mha(x[b:b + 1], weights(E).t, 1)[0][0, :n]
        changed = int((padded != want[b, :n]).any(-1).sum())
        print(f"{case_id(case)} frame {b}: {changed} of {n} valid rows change")
        assert changed > 0, f"frame {b} (len {n}): this padding would not show a missing mask; change the seed"
