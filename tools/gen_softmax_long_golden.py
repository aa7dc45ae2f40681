#!/usr/bin/env python3
"""Golden rows of the integer softmax on LONG rows, by running the reference in the build container (like
tools/gen_golden.py, whose reference path this imports: never on the GPU box).

tests/golden/softmax_rows.npz and softmax_inverse.npz stop at 128 keys, i.e. at row sums of 32 768.  A row of the long
attention (ita_long_attn_kernel.h) has up to 65 536 keys; its denominator  inv = floor(255 * 2^16 / sum)  keeps
inv >> 8 non-zero up to sum = 65 280 and the probabilities of every key are 0 beyond.  This file pins the reference's
IntegerApproximatedSoftmaxFn (models/ITA/QAT/ITA_softmax.py:19-73, quantized branch) there:

    x256 / y256     rows of 256 int8 logits and the reference's uint8 probabilities: sums of exactly 32 768, 32 769,
                    65 216, 65 280, 65 281 and 65 536, each at two different row maxima, every one of them with single keys lowered by
                    1 .. 9, and random rows
    sum256          the row sums (sum of 256 >> (max - x)) the rows were built for, -1 for the random rows
    x8192 / y8192   rows of 8192 logits: sums of 65 279, 2^16 + 1, 2^20, 2^21, and one random row
    sum8192

A sum of 65 279 cannot occur in a row of 256 keys: a key at the maximum contributes 256 and any other key 256 - d with d
in {128, 192, 224, ..., 255, 256}, so 65 536 - sum is 0, one such d, or at least 128 + 128; 257 is none of these.  The
nearest sum below 65 280 that 256 keys reach is 65 216 (d = 128 + 192); 65 279 itself is pinned at 8192 keys.

Every logit is at least -127, so that a test can produce a row as the logits -c_j of keys c_j in [-127, 127].
Only DATA is written.  Usage:  python tools/gen_softmax_long_golden.py [--out tests/golden]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as gg  # noqa: E402  (puts the reference on sys.path)

SUMS_256 = (32768, 32769, 65216, 65280, 65281, 65536)
SUMS_8192 = (65279, (1 << 16) + 1, 1 << 20, 1 << 21)


def shifts_for(total, n):
    """n shifts (0: the maximum; 9: contributes nothing) with sum of 256 >> shift == total, at least one of them 0"""
    assert 256 <= total <= 256 * n
    counts, rest = [1] + [0] * 8, total - 256
    for s in range(9):
        c = rest // (256 >> s)
        counts[s] += c
        rest -= c * (256 >> s)
    assert rest == 0 and sum(counts) <= n, (total, n, counts)
    sh = np.full(n, 9, np.int64)
    sh[:sum(counts)] = np.repeat(np.arange(9), counts)
    return sh


def row_of(total, n, top, rs):
    """a row of n logits with the maximum `top` and the row sum `total`, keys in a seeded random order"""
    x = top - rs.permutation(shifts_for(total, n))
    assert x.min() >= -127
    return x.astype(np.int8)


def row_sum(x):
    d = x.astype(np.int64).max() - x.astype(np.int64)
    return int(np.where(d > 31, 0, 256 >> np.minimum(d, 31)).sum())


def reference(x):
    from models.ITA.QAT.ITA_softmax import IntegerApproximatedSoftmax
    sm = IntegerApproximatedSoftmax(dim=-1)
    q = torch._make_per_tensor_quantized_tensor(torch.from_numpy(x).reshape(1, 1, *x.shape), scale=0.1, zero_point=0)
    y = sm(q)
    assert y.dtype == torch.quint8 and y.q_zero_point() == 0
    return y.int_repr().numpy().reshape(x.shape)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(gg.REPO, "tests", "golden"))
    a = ap.parse_args()
    rs = np.random.RandomState(256)
    rows, sums = [], []
    for total in SUMS_256:
        for top in (127, -40):
            base = row_of(total, 256, top, rs)
            assert row_sum(base) == total
            rows.append(base); sums.append(total)
        base = rows[-2]                       # neighbours: one key at the maximum (where it is not the only one) and one
        at_max, below = np.flatnonzero(base == base.max()), np.flatnonzero(base < base.max())   # below it, lowered by 1 .. 9
        for lower in range(1, 10):
            for keys in (at_max if len(at_max) > 1 else (), below):
                if len(keys):
                    r = base.copy()
                    r[keys[lower % len(keys)]] -= lower
                    rows.append(r); sums.append(row_sum(r))
    for _ in range(4):
        rows.append(rs.randint(-127, 128, size=256).astype(np.int8)); sums.append(-1)
    for sc in (2, 6, 20):
        rows.append(np.clip(np.round(rs.standard_normal(256) * sc), -127, 127).astype(np.int8)); sums.append(-1)
    x256 = np.stack(rows).astype(np.int8)
    rows8, sums8 = [], []
    for total, top in zip(SUMS_8192, (127, 5, 127, -60)):
        rows8.append(row_of(total, 8192, top, rs)); sums8.append(total)
        assert row_sum(rows8[-1]) == total
    rows8.append(np.clip(np.round(rs.standard_normal(8192) * 3), -127, 127).astype(np.int8)); sums8.append(-1)
    x8192 = np.stack(rows8).astype(np.int8)
    assert x256.min() >= -127 and x8192.min() >= -127
    path = os.path.join(a.out, "softmax_long_rows.npz")
    np.savez_compressed(path, x256=x256, y256=reference(x256), sum256=np.array(sums, np.int64),
                        x8192=x8192, y8192=reference(x8192), sum8192=np.array(sums8, np.int64),
                        **{"meta.torch": np.array(torch.__version__)})
    print("wrote", path, x256.shape, x8192.shape, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
