"""attention_hist_f32_ref.hist_f32 against a per-element Python loop of the definition in include/ita_mi355x.h
(ita_mha_long_f32_hist), at S = 128 on a flat row, a row with one dominant key and random rows."""
import numpy as np
import pytest

from drone_oa_iree_vit_accelerator_amd import attention_hist_f32_ref as ahr
from drone_oa_iree_vit_accelerator_amd import attention_stats_f32_ref as asr
from oracle import oracle

S = 128
f32 = np.float32


def _logits(kind):
    rs = np.random.RandomState(3)
    if kind == "flat":
        return np.full((1, S, S), 3.25, f32)
    if kind == "dominant":                  # key (i * 5) % S of row i is 200 above the rest: d >= 87 for all others
        s = (rs.standard_normal((1, S, S)) * 3 - 90).astype(f32)
        s[0, np.arange(S), (np.arange(S) * 5) % S] += f32(200)
        return s
    return (rs.standard_normal((2, S, S)) * 40).astype(f32)     # |logit| reaches ~160: both logits_out counters


@pytest.mark.parametrize("kind,scale", [("flat", 1.0), ("dominant", 0.5), ("random", 1.0), ("random", 3.7)])
def test_hist_f32_against_a_loop_over_the_elements(kind, scale):
    s = _logits(kind)
    m = s.max(-1)
    l = asr.expf(s - m[..., None]).sum(-1, dtype=f32)
    got = ahr.hist_f32(s, m, l, scale)
    expf = oracle.lib().ita_oracle_expf
    want = {k: np.zeros((s.shape[0], 256), np.int64) for k in ("logits", "shifts", "probs")}
    out = np.zeros((s.shape[0], 2), np.int64)
    for b, i, j in np.ndindex(*s.shape):
        r = np.rint(s[b, i, j] * f32(scale))
        want["logits"][b, int(min(max(r, -128), 127)) + 128] += 1
        out[b] += (r < -128, r > 127)
        want["shifts"][b, int(min(np.rint((m[b, i] - s[b, i, j]) * f32(scale)), 255))] += 1
        p = f32(expf(float(s[b, i, j] - m[b, i]))) * (f32(1.0) / l[b, i])
        assert p.dtype == f32
        want["probs"][b, int(p.view(np.uint32)) >> 23] += 1
    for k, v in want.items():
        np.testing.assert_array_equal(got[k], v, err_msg=k)
        assert got[k].dtype == np.int64 and (got[k].sum(-1) == S * S).all(), k
    np.testing.assert_array_equal(got["logits_out"], out)
    np.testing.assert_array_equal(got["range"], np.stack([s.min((1, 2)), s.max((1, 2))], -1))
    assert got["range"].dtype == f32
    if kind == "flat":          # one hot bin per histogram: r = 3, d = 0, p = 1 / 128
        assert got["logits"][0, 131] == got["shifts"][0, 0] == got["probs"][0, 120] == S * S
    if kind == "random" and scale == 1.0:
        assert (got["logits_out"] > 0).all()
