"""ita_mha_long_int8_hist at S = 65 536, B = 1, on the int8 vocabulary frames of long_limits_common: 65 536 tokens drawn
from 512 distinct ones, so the histograms of the 2^32 entries follow exactly from the 512 x 512 matrix of the
representatives (attention_hist_ref.hist_from_classes: milliseconds of numpy).  Every histogram sums to exactly 2^32 and
bins exceed 2^31, so a 32-bit total anywhere in the kernel or the binding shows."""
import numpy as np
import pytest

from drone_oa_iree_vit_accelerator_amd import attention_hist_ref as ahr
from drone_oa_iree_vit_accelerator_amd import host
from gpu_support import cu, to_numpy
from long_cases import long_case
import long_hist_common as lhc
import long_limits_common as llc

pytestmark = pytest.mark.gpu

S = 65536


@pytest.mark.parametrize("name,l", llc.INT8_MODELS)
def test_65536_keys_against_the_class_form(name, l):
    case = long_case(name)
    t, blob = case.t, case.blob
    x, reps, cls, counts = llc.int8_vocab_frame(name, l, S)
    assert x.shape[:2] == (1, S) and len(reps) == 512 and int(counts.sum()) == S
    want = ahr.hist_from_classes(x[0, reps], counts, t, l)
    for k in ("logits", "shifts", "probs"):
        assert int(want[k].sum()) == 1 << 32, k
    assert max(int(want[k].max()) for k in ("logits", "shifts", "probs")) > 1 << 31
    eng = host.Engine(blob, device=0)
    got = to_numpy(eng.attention_histograms_long(cu(x), l))
    eng.close()
    assert tuple(got) == lhc.NAMES
    for k in lhc.NAMES:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{name} layer {l} {k}")
