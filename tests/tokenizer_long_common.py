"""The long-sequence tokenizer's bit-exact expectation, composed from the definition's blended patches and two oracle
functions (test_tokenizer_long_cpu.py says why these chains); shared by the CPU and the GPU test.  CPU only."""
import functools

import numpy as np

from drone_oa_iree_vit_accelerator_amd import synth
from drone_oa_iree_vit_accelerator_amd import tokenizer_long_ref as tl


@functools.lru_cache(maxsize=None)
def tok_params(E, seed=0):
    """(conv_w (E, 49), conv_b, ln_w, ln_b) of synth.float_params(seed, E); read-only"""
    fp = synth.float_params(seed, E=E)
    return (fp["tokenizer.conv.weight"].reshape(E, 49), fp["tokenizer.conv.bias"], fp["tokenizer.norm.weight"],
            fp["tokenizer.norm.bias"])


def composed(oracle, frames, tok_h, tok_w, E, depth_scale=None, seed=0):
    """the definition's tokens (B, tok_h * tok_w, E) float32"""
    cw, cb, lw, lb = tok_params(E, seed)
    pb = tl.blend_patches(frames, tok_h, tok_w, depth_scale)
    pre = oracle.linear_f32(pb.reshape(-1, 49), cw, cb)
    return oracle.add_ln(pre, np.zeros_like(pre), lw, lb).reshape(pb.shape[0], tok_h * tok_w, E)
