"""A condition on the ragged float tests' INPUTS, not a second implementation: with the padding ragged_f32_cases.inputs
gives, float64 attention (and the float64 layer) over the PADDED frame misses the bound against the reference on the
unpadded one in a valid row, for every frame shorter than S_pad (the empty frame has no valid row) -- so a kernel that
ignored the lengths cannot pass test_gpu_long_f32_ragged.py.  Also: the two entries are declared and registered."""
import ctypes
import os
import re

import numpy as np
import pytest

from drone_oa_iree_vit_accelerator_amd import host
import long_f32_common as lc
from ragged_f32_cases import CASES, case_id, inputs, refs


@pytest.mark.parametrize("case", CASES, ids=case_id)
@pytest.mark.parametrize("E", [64, 128])
def test_ignored_lengths_miss_the_bound(E, case):
    (S_pad, lens), fp = case, lc.case(E)[0]
    for what, f64 in (("attn", lc.attn64), ("layer", lc.layer64))[:2 if case in (CASES[7], CASES[-1]) else 1]:   # the layer test's cases
        for rev, layer in ((r, l) for r in (False, True) for l in range(lc.LAYERS[E])):
            x = inputs(E, S_pad, lens, rev)
            for b, (n, (want, e_torch)) in enumerate(zip(lens, refs(what, E, S_pad, lens, rev, layer))):
                if n not in (0, S_pad):
                    d = float(np.abs(f64(x[b:b + 1], fp, layer)[0, :n] - want).max())
                    print(f"{what} {case_id(case)} rev={rev} layer {layer} frame {b}: {d:.3e}, bound {lc.bound(e_torch):.3e}")
                    assert d > lc.bound(e_torch), f"{what} frame {b} (len {n}): this padding would not show ignored lengths"


def test_entries_declared_and_registered():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ita_mi355x.h")).read()
    vp, i = ctypes.c_void_p, ctypes.c_int
    for name in ("ita_mha_long_f32_ragged", "ita_encoder_layer_long_f32_ragged"):
        assert re.search(r"\bint\s+%s\s*\(\s*ita_handle\s+h,\s*int\s+layer,\s*const\s+float\*\s*x_dev,\s*float\*\s*y_dev,\s*int\s+batch,"
                         r"\s*int\s+seq_stride,\s*const\s+int\*\s*lens_dev,\s*void\*\s*stream\)" % name, hdr), name
        assert name in host.EXPORTED_SYMBOLS and getattr(host.lib(), name).argtypes == [vp, i, vp, vp, i, i, vp, vp], name
