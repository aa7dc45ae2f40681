"""The ragged long-attention tests' case table, inputs and definition, shared by the CPU and the GPU test.  CPU only.

Inputs: valid tokens are seeded randn; the padding rows are seeded normal noise at 4 x that amplitude -- not zeros, which
quantise to code 0 and hide a missing mask (test_long_ragged_cpu.py holds the inputs to that)."""
import functools

import numpy as np

from drone_oa_iree_vit_accelerator_amd import mha_heads_ref as ref
from long_cases import long_case

FIXTURE = {64: "vitlstm_E64_seed0_B2", 128: "vit2l_E128_s0_B2"}     # the FAST and the exact requantisation form
# (S_pad, lens): one tile with 1, 127, 128 keys; two tiles; three (the ring wraps); six; a mixed batch with a full frame,
# an empty one and one that ends on a tile edge
CASES = [(128, (1,)), (128, (127,)), (128, (128,)), (256, (129,)), (256, (200,)), (384, (257,)), (768, (641,)),
         (384, (384, 129, 1, 0, 256))]
case_id = lambda c: f"{c[0]}-{'_'.join(map(str, c[1]))}"


weights = lambda E: long_case(FIXTURE[E])


@functools.lru_cache(maxsize=None)
def inputs(E, S_pad, lens, seed=7):
    """x (B, S_pad, E) f32, read-only"""
    rs = np.random.RandomState(seed + S_pad + sum(lens))
    x = (4.0 * rs.standard_normal((len(lens), S_pad, E))).astype(np.float32)
    for b, n in enumerate(lens):
        x[b, :n] = rs.standard_normal((n, E)).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def definition(E, S_pad, lens):
    """(B, S_pad, E): attention of every frame's valid tokens alone, mha_heads_ref.mha at H = 1, zeros behind; read-only"""
    x, y = inputs(E, S_pad, lens), np.zeros((len(lens), S_pad, E), np.float32)
    for b, n in enumerate(lens):
        if n:
            y[b, :n] = ref.mha(x[b:b + 1, :n], weights(E).t, 1)[0][0]
    y.setflags(write=False)
    return y
