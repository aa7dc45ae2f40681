"""Shared by test_long_propagate_cpu.py and test_gpu_long_propagate.py: the blobs, the weight builders and the cached
definitions of the weighted column sums (attention_propagate_ref) and the rollout (attention_rollout_ref).  CPU only.

Weights (B, 64, S) int8 of one (S, B): random in [-127, 127], except
    row 0          frame 0 random, frame 1 equal to -128 everywhere, frame 2 one-hot at token S - 1   (what R = 1 runs)
    rows 8 .. 15   all zero | all 127 | all -127 | one-hot at tokens 0, 127, 128 % S, S - 1 | -128 everywhere,
                   rotated by the frame index so that the frames differ
The sums are linear in the weight rows, so a call with the first R rows is held to the first R rows of ONE definition
per (blob, S): R = 1, 16, 17 (one row in the second group of 16) and 64 share it, and B = 1 is its frame 0."""
import functools

import numpy as np

from drone_oa_iree_vit_accelerator_amd import attention_propagate_ref as apr
import long_taps_common as ltc
from long_cases import long_case, tokens

FIXTURES = ("vitlstm_E64_seed0_B2", "blocks_E128_seed0_B1")
CRAFTED = ("fast", "exact")
BLOBS = FIXTURES + CRAFTED
SEQS = (128, 256, 384, 1024)        # one tile, both ring slots, an odd tile count, many tiles
BATCHES = (1, 3)
ROWS = (1, 16, 17, 64)
ROLLOUT_BLOBS = ("vit2l_E128_s0_B2", "vitlstm_E64_seed0_B2")     # two layers, one layer


@functools.lru_cache(maxsize=None)
def blob_case(name):
    """(E, attention tensors, blob) of a fixture or a crafted form; read-only"""
    if name in CRAFTED:
        E, t, _ = ltc.crafted(name)
        return E, t, ltc.blob(name)
    c = long_case(name)
    return c.E, c.t, c.blob


def one_hot(S, token, value=1):
    w = np.zeros(S, np.int8)
    w[token] = value
    return w


def specials(S):
    """the eight special rows"""
    return [np.zeros(S, np.int8), np.full(S, 127, np.int8), np.full(S, -127, np.int8), one_hot(S, 0), one_hot(S, 127),
            one_hot(S, 128 % S), one_hot(S, S - 1), np.full(S, -128, np.int8)]


def weights(S, B, seed=0):
    """(B, 64, S) int8, as the module docstring says"""
    w = np.random.RandomState(1000 * S + B + seed).randint(-127, 128, size=(B, 64, S)).astype(np.int8)
    sp = specials(S)
    for b in range(B):
        for k in range(8):
            w[b, 8 + k] = sp[(k + b) % 8]
    if B > 1:
        w[1, 0] = -128
    if B > 2:
        w[2, 0] = one_hot(S, S - 1)
    return w


def frames(name, S, B):
    """(B, S, E) f32: random structured tokens for a fixture; for a crafted form frames whose queries all see one fixture
    row (rows 0 .. B - 1 of x256 tiled to S keys)"""
    E, t, _ = blob_case(name)
    if name in CRAFTED:
        rows = np.tile(ltc.fixture()["x256"][:B], (1, (S + 255) // 256))[:, :S]
        return ltc.frames_for(name, rows)
    return tokens(S + B, B, S, E, t)


@functools.lru_cache(maxsize=None)
def expected(name, S):
    """(x (3, S, E), w (3, 64, S), the definition's (3, 64, S) int32) of one case: computed once, read-only"""
    _, t, _ = blob_case(name)
    x, w = frames(name, S, 3), weights(S, 3)
    want = apr.propagate(x, t, w)
    for a in (x, w, want):
        a.setflags(write=False)
    return x, w, want
