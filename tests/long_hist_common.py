"""Shared by test_long_hist_cpu.py, test_gpu_long_hist.py and test_gpu_long_hist_limits.py: the fixtures, shapes and inputs of
the long-sequence histogram tests (ita_mha_long_int8_hist) and the definition's results on them, computed once.  CPU only.

Fixtures: the four forms of test_gpu_long_layer.py with long_cases' long_case / long_f32 inputs -- exact and FAST at E = 64 and at
E = 128, the FAST E = 128 blob on both layers.  Shapes (S, B): (128, 3) one key tile; (256, 2) / (384, 2) even and odd tile
counts, so the ring-slot parity differs between the two sweeps; B > 1 the frame strides; (1024, 1) a longer sum."""
import functools

import numpy as np

from drone_oa_iree_vit_accelerator_amd import attention_hist_ref as ahr
import softmax_clamp_common as scc
from long_cases import long_case, long_f32

FIXTURES = (("blocks_E64_seed2_B1", 0), ("vitlstm_E64_seed0_B2", 0), ("blocks_E128_seed0_B1", 0),
            ("vit2l_us_E128_s1_B2", 0), ("vit2l_us_E128_s1_B2", 1))
FAST = {"blocks_E64_seed2_B1": False, "vitlstm_E64_seed0_B2": True, "blocks_E128_seed0_B1": False, "vit2l_us_E128_s1_B2": True}
SHAPES = [(128, 3), (256, 2), (384, 2), (1024, 1)]
BIG = ("vitlstm_E64_seed0_B2", 0, 8192, 1)
NAMES = ahr.NAMES
DTYPES = dict(logits=np.int64, logits_out=np.int64, acc_range=np.int32, shifts=np.int64, probs=np.int64)
WIDTH = dict(logits=256, logits_out=2, acc_range=2, shifts=256, probs=256)
CLAMP_FORMS, CLAMP_S = ("fast", "exact"), scc.LONG_S


def _frozen(x, h):
    x.setflags(write=False)
    for v in h.values():
        v.setflags(write=False)
    return x, h


@functools.lru_cache(maxsize=None)
def expected(name, l, S, B):
    """(x (B, S, E) f32, attention_hist_ref.hist of it) of one case; read-only"""
    case = long_case(name)
    E, t = case.E, case.t
    x = long_f32(S + B, B, S, E, t, l)
    return _frozen(x, ahr.hist(x, t, l))


@functools.lru_cache(maxsize=None)
def clamp_expected(form, S):
    """(x (3, S, E) f32, the definition's histograms, raw (3, S, S) the wanted raw logits, rows, d) of the crafted frames of
    softmax_clamp_common at S keys; read-only"""
    rows, d = scc.rows_long(S)
    x = scc.frames_for(form, rows, d)
    return _frozen(x, ahr.hist(x, scc.crafted(form)[1])) + (scc.wanted_raw(rows, d)[:, 0],)


def conditions(h):
    """what the GPU tests rely on, over the frames of a case's result h: >= 64 non-empty logit bins, shifts above 15 and
    above 31 present, >= 128 non-empty probability bins -> (logit bins, share of shifts above 31, probability bins)"""
    lb = int(np.count_nonzero(h["logits"].sum(0)))
    pb = int(np.count_nonzero(h["probs"].sum(0)))
    s16, s32 = int(h["shifts"][:, 16:].sum()), int(h["shifts"][:, 32:].sum())
    assert lb >= 64 and s16 > 0 and s32 > 0 and pb >= 128, (lb, s16, s32, pb)
    return lb, s32 / int(h["shifts"].sum()), pb
