"""The inputs of test_gpu_float_flat.py are what they claim, in float64 on the CPU: how many keys of a softmax row carry
weight (probability above 1e-4) with q_proj of the layer under test times s, next to the stock weights (s = 1).

Measured, keys above 1e-4 per row as min / median / max over the rows of all layers, and e_torch = max |torch f32 - float64|
of the attention block (the test prints the figures of every case):

  plain rows, S = 128   s = 0      128 / 128 / 128          e_torch 6.8e-8 .. 9.1e-8
                        s = 1/64   128 / 128 / 128                  1.4e-7 .. 1.9e-7
                        s = 1/8    1 / 22 .. 27 / 57 .. 66          3.1e-6 .. 5.2e-6
                        s = 1      1 / 1 / 6 .. 8                   1.9e-5 .. 3.4e-5
  ramp rows, S = 128    s = 1/64   126 .. 127 / 128 / 128           4.3e-7 .. 7.2e-7
                        s = 1/8    1 / 11 .. 16 / 106 .. 110        5.4e-6 .. 9.5e-6
  S = 256, 384          s = 1/64   >= 368 of 384, 251 of 256 / S / S
                        s = 1/8    1 / 17 .. 44 / 87 .. 262
                        s = 1      1 / 1 .. 2 / 7 .. 10

So the three conditions "all S keys at s = 0 and 1/64, a median of at least 16 at 1/8, at most 4 at s = 1" hold on the plain
rows at S = 128, where they were first measured, and are asserted there as they stand.  They do not all carry over to the
ramped rows and to S > 128, and the reason is in the inputs: the ramp multiplies token t by r_t in [0.5, 1.5], so the logit
of (query i, key j) grows by about r_i r_j, up to 2.25 -- a ramped row at s = 1/64 is as peaked as a plain one at 1/28 --
and with S keys the uniform probability 1 / S itself comes within 26 x of the 1e-4 mark at S = 384.  What is asserted there
instead: all S keys at s = 0 (exact: every probability is 1 / S), at s = 1/64 the median row has all S keys and every row at
least 7 S / 8, at s = 1/8 the median row has at least 8 keys, twice what the stock weights allow (at most 4).

What a fault in the handling of the non-dominant keys costs, as a float64 mutation of attn64 on the plain rows at S = 128
(max over a row's outputs of |mutant - attn64|; "rows" = share of rows moved by more than the test's bound):

                                         s = 1/64                           s = 1 (stock)
  context GEMM skips key tile 7          median row 3.3e-2 .. 4.5e-2, 100 % of rows    median row 2e-15 .. 1e-12, 18 .. 26 % of rows
  key 100 missing from the row sum       median row 1.0e-3 .. 1.2e-3, 100 %            median row 0, 1 .. 2 %
  V rows of keys 5 and 6 swapped         median row 3.7e-3 .. 5.2e-3, 100 %            median row 0, 1 .. 3 %
  (bound 1e-5 at s = 1/64: the floor; 5.6e-5 .. 1.0e-4 at s = 1)

With the stock weights such a fault shows only on the rows whose one dominant key it happens to touch; on the flat rows
every row of every frame misses the bound by two to three orders of magnitude.  test_mutations_show_on_flat_rows asserts
the first line."""
import numpy as np
import pytest

import float_flat_common as fc
import long_f32_common as lc
from long_f32_common import LAYERS

CASES = [(E, l) for E in sorted(LAYERS) for l in range(LAYERS[E])]


def _counts(E, l, s, kind, S, B):
    n = fc.keys_per_row(lc.inputs(kind, E, S, B), fc.case(E, l, s)[0], l)
    e = fc.attn_ref(kind, E, S, B, l, s)[1]
    print(f"E={E} layer {l} s={fc.label(s) if s != 1 else '1'} {kind} S={S} B={B}: keys above {fc.P_MIN:g} per row "
          f"min {n.min()} median {np.median(n):g} max {n.max()}, e_torch {e:.2e}")
    return n


@pytest.mark.parametrize("E,l", CASES)
def test_plain_rows_at_128_keys(E, l):
    S, B = fc.SHORT
    for s in (0.0, 1.0 / 64):
        assert (_counts(E, l, s, "plain", S, B) == S).all(), s
    assert np.median(_counts(E, l, 1.0 / 8, "plain", S, B)) >= 16
    assert np.median(_counts(E, l, 1.0, "plain", S, B)) <= 4   # the gap: with the stock weights P V is a gather


@pytest.mark.parametrize("E,l", CASES)
@pytest.mark.parametrize("kind,S,B", [("ramp",) + fc.SHORT] + [(k,) + sb for k in fc.KINDS for sb in fc.LONG])
def test_ramped_and_long_rows(E, l, kind, S, B):
    assert (_counts(E, l, 0.0, kind, S, B) == S).all()
    n = _counts(E, l, 1.0 / 64, kind, S, B)
    assert np.median(n) == S and n.min() >= 7 * S // 8
    assert np.median(_counts(E, l, 1.0 / 8, kind, S, B)) >= 8
    assert np.median(_counts(E, l, 1.0, kind, S, B)) <= 4


@pytest.mark.parametrize("E,l", CASES)
def test_exact_rows_at_scale_zero(E, l):
    """s = 0: Q is exactly zero in float32 as well (0 * w summed onto a zero bias), so every probability is 1 / S"""
    fp = fc.case(E, l, 0.0)[0]
    assert not fp[f"attention_blocks.{l}.q_proj.weight"].any() and not fp[f"attention_blocks.{l}.q_proj.bias"].any()
    for other in range(LAYERS[E]):
        if other != l:
            name = f"attention_blocks.{other}.q_proj.weight"
            assert np.array_equal(fp[name], lc.case(E)[0][name])
    p, _ = lc.probs64(lc.inputs("plain", E, *fc.SHORT), fp, l)
    assert (p == 1.0 / fc.SHORT[0]).all()


@pytest.mark.parametrize("E,l", CASES)
def test_mutations_show_on_flat_rows(E, l):
    """the context GEMM without key tile 7, in float64: at s = 1/64 every row moves by more than 100 x the bound; with the
    stock weights the median row does not reach it"""
    S, B = fc.SHORT
    x = lc.inputs("plain", E, S, B)
    moved = {}
    for s in (1.0 / 64, 1.0):
        want, e = fc.attn_ref("plain", E, S, B, l, s)
        d = np.abs(fc.attn64_without_key_tile(x, fc.case(E, l, s)[0], l, 7) - want).max(-1)
        moved[s] = d / lc.bound(e)
        print(f"E={E} layer {l} s={s:g}: skip key tile 7 moves a row by min {d.min():.2e} median {np.median(d):.2e} max {d.max():.2e}; "
              f"bound {lc.bound(e):.1e}, rows over it {100 * (moved[s] > 1).mean():.0f} %")
    assert moved[1.0 / 64].min() > 100
    assert np.median(moved[1.0]) < 1
