"""Long float attention histograms on the MI355X: ita_mha_long_f32_hist (Engine.attention_histograms_long_f32).

1. Bit for bit against attention_hist_f32_ref.hist_f32 of the kernels' own logits, row maxima and row sums (the taps of all
   rows, S <= 1024).  Inputs: 'ln' = the ln_like activations with the stock blob (|logit| reaches ~230; at SCALE both
   logits_out counters are non-zero) and 'flat0' = q_proj times 0 (float_flat_common): every logit 0, d = 0, p = 1 / S,
   one hot bin per histogram.  S = 128 one query tile, 256 two workgroups per frame and the ring reused across the
   sweeps, 1024 the largest fully tappable shape.
2. Against float64 from the parameters on 'flat8' (q_proj times 1 / 8: logits within ~ +-30, gaps and exponents spread over
   many bins) at S = 256: an element may change its bin only where its float64 value lies within tol of a bin edge.
   tol is measured in the test from the taps: the largest deviation of their logits (twice that for a gap, which has two
   of them), and of their probabilities relatively, from float64; plus 2^-15 of a bin for the f32 roundings of the
   product with scale and of the subtraction (|value| <= 256 at an edge: two roundings of 2^-24 * 256).  On the CPU
   the f32 model of the kernel (long_f32_stats_common.logits_f32) gives tol 4.9e-6 (logits) and 8.1e-6 (relative, p), no
   excess at any edge and allowed migrations of 0.02 % of S^2 summed over all edges, E = 64 and 128 alike; the test
   asserts < 1 %.
3. One captured call replayed; 4. the refusals."""
import numpy as np
import pytest
import torch

from drone_oa_iree_vit_accelerator_amd import attention_hist_f32_ref as ahr
from drone_oa_iree_vit_accelerator_amd import host
from gpu_support import INVALID, UNSUPPORTED, Canaries, captured_replays, cu, engine_pool, refused, same_bits, to_numpy
from long_cases import long_case
import float_flat_common as ffc
import long_f32_common as lc

pytestmark = pytest.mark.gpu

NAMES = host.LONG_F32_HIST
SCALE = {"ln": 1.0, "flat0": 1.0, "flat8": 4.0}
Q_SCALE = {"ln": 1, "flat0": 0.0, "flat8": 1.0 / 8}
ROW_TAPS = ("logits", "probs", "row_max", "row_sum")


@pytest.fixture(scope="module")
def engines():
    yield from engine_pool(lambda kind, E: ffc.case(E, 0, Q_SCALE[kind])[1])


def _taps(eng, x):
    return to_numpy(eng._long_f32_taps(x, list(range(x.shape[1])), 0, ROW_TAPS)[1])


def _canaries(B):
    return Canaries({k: ((B, 2 if k in ("logits_out", "range") else 256), torch.float32 if k == "range" else torch.int64) for k in NAMES})


def _call(eng, x, st, S=None, scale=1.0):
    host._chk(host.lib().ita_mha_long_f32_hist(eng._h, 0, x.data_ptr() if x is not None else None, 1 if x is None else x.shape[0],
                                               (256 if x is None else x.shape[1]) if S is None else S, scale,
                                               host.C.byref(st) if st is not None else None, host._stream_ptr(eng.device)))


@pytest.mark.parametrize("E", [64, 128])
@pytest.mark.parametrize("S", [128, 256, 1024])
@pytest.mark.parametrize("kind", ["ln", "flat0"])
def test_bit_for_bit_against_the_kernels_own_matrix(engines, kind, S, E):
    B, scale = 2, SCALE[kind]
    eng = engines(kind, E)
    x = cu(lc.inputs("plain", E, S, B))
    got = eng.attention_histograms_long_f32(x, 0, scale)
    assert tuple(got) == NAMES and torch.equal(x, cu(lc.inputs("plain", E, S, B))), "x was written to"
    tp = _taps(eng, x)
    ref = ahr.hist_f32(tp["logits"], tp["row_max"], tp["row_sum"], scale)
    g = to_numpy(got)
    for k in NAMES:
        assert g[k].dtype == ref[k].dtype and np.array_equal(g[k], ref[k]), (k, g[k], ref[k])
    assert all((g[k].sum(-1) == S * S).all() for k in ("logits", "shifts", "probs"))
    if kind == "ln":
        assert (g["logits_out"] > 0).all(), "SCALE must put logits on both sides of the int8 range"
    else:
        assert all((g[k].max(-1) == S * S).all() for k in ("logits", "shifts", "probs")), "flat rows: one hot bin each"
    # the same bytes on a second call, for a frame alone, and for a subset of the outputs, which writes nothing else
    assert same_bits(eng.attention_histograms_long_f32(x, 0, scale), got, NAMES)
    for b in range(B):
        alone = eng.attention_histograms_long_f32(x[b:b + 1].contiguous(), 0, scale)
        assert same_bits(alone, {k: v[b:b + 1] for k, v in got.items()}, NAMES), f"frame {b} alone differs"
    for want in [(k,) for k in NAMES] + [("logits_out", "range"), ("shifts", "probs")]:
        c = _canaries(B)
        _call(eng, x, host._MhaLongF32Hist(**c.ptrs(want)), scale=scale)
        torch.cuda.synchronize()
        assert same_bits(c.views(), got, want), want
        c.assert_untouched(written=want)


def migrations(h32, h64, v64, edges, tol, relative=False):
    """h32, h64: (256,) counts; v64: the float64 values that h64 bins; edges[k]: the value between bin k and bin k + 1.
    -> (worst excess of |cumulative h32 - cumulative h64| over the float64 values within tol of the edge, sum of those
    allowances over all edges)"""
    v = np.sort(v64.ravel())
    lo, hi = (edges * (1 - tol), edges * (1 + tol)) if relative else (edges - tol, edges + tol)
    near = np.searchsorted(v, hi, "right") - np.searchsorted(v, lo, "left")
    diff = np.abs(np.cumsum(h32)[:len(edges)] - np.cumsum(h64)[:len(edges)])
    return int((diff - near).max()), int(near.sum())


def check_against_float64(g, t64, taps, scale, S):
    """g: the GPU's histograms, t64: ahr.hist64, taps: the kernels' own matrix (tol is measured on it).  -> report"""
    tol_s = float(np.abs(taps["logits"] - t64["s"]).max())
    live = t64["p"] > 2.0 ** -100
    tol_p = float(np.abs(taps["probs"][live] / t64["p"][live] - 1).max())
    half = np.arange(255) + 0.5                 # rint: the edge between bins k and k + 1, in units of a bin
    rounding = 2.0 ** -15
    out = dict(tol_logit=tol_s, tol_prob_rel=tol_p)
    for b in range(g["logits"].shape[0]):
        for k, v64, edges, tol, rel in (("logits", t64["s"][b] * scale, half - 128, tol_s * scale + rounding, False),
                                        ("shifts", t64["d"][b] * scale, half, 2 * tol_s * scale + rounding, False),
                                        ("probs", t64["p"][b], 2.0 ** (np.arange(255) - 126.0), tol_p + 2.0 ** -22, True)):
            excess, allowed = migrations(g[k][b], t64[k][b], v64, edges, tol, rel)
            out[f"{k}[{b}]"] = (excess, allowed)
    return out


@pytest.mark.parametrize("E", [64, 128])
def test_against_float64_from_the_parameters(engines, E):
    S, B, scale = 256, 2, SCALE["flat8"]
    eng = engines("flat8", E)
    xn = lc.inputs("plain", E, S, B)
    g = to_numpy(eng.attention_histograms_long_f32(cu(xn), 0, scale))
    t64 = ahr.hist64(xn, ffc.case(E, 0, Q_SCALE["flat8"])[0], scale)
    rep = check_against_float64(g, t64, _taps(eng, cu(xn)), scale, S)
    print(f"E={E}: {rep}")
    pairs = [v for k, v in rep.items() if k.endswith("]")]
    for b in range(B):
        assert sum(v[1] for k, v in rep.items() if k.endswith(f"[{b}]")) < 0.01 * S * S, "the case allows too many migrations"
    assert max(e for e, _ in pairs) <= 0, rep
    assert np.abs(g["range"] - t64["range"]).max() <= rep["tol_logit"]
    assert (np.abs(g["logits_out"] - t64["logits_out"]).sum(-1) <= rep["logits[0]"][1] + rep["logits[1]"][1]).all()


def test_captured_call_replays(engines):
    S, B, E = 256, 2, 64
    eng = engines("ln", E)
    x = cu(lc.inputs("plain", E, S, B))
    c = _canaries(B)
    st = host._MhaLongF32Hist(**c.ptrs())
    captured_replays(lambda: eng.attention_histograms_long_f32(x, 0, SCALE["ln"]), lambda: _call(eng, x, st, scale=SCALE["ln"]), c, NAMES)


def test_refusals_before_any_launch(engines):
    def no(eng, status, seq_len=None, null_x=False, want=NAMES, skew=None, scale=1.0):
        x = torch.zeros((1, 256, eng.E), dtype=torch.float32, device="cuda")
        c = _canaries(1)
        st = host._MhaLongF32Hist(**{k: c.ptr(k, (2 if k == "range" else 4) if k == skew else 0) for k in want})
        refused(lambda: _call(eng, None if null_x else x, st, seq_len, scale), c, status)

    ei = host.Engine(long_case("vitlstm_E64_seed0_B2").blob, device=0)
    assert ei.attn_kind(0) == host.ATTN_INT8
    no(ei, UNSUPPORTED)
    assert "ita_mha_long_int8_hist" in host.lib().ita_error_string().decode()
    ei.close()
    eng = engines("ln", 64)
    no(eng, UNSUPPORTED, seq_len=192)
    no(eng, INVALID, null_x=True)
    no(eng, INVALID, want=())
    for k in NAMES:
        no(eng, INVALID, skew=k)
    for scale in (0.0, -1.0, float("inf"), float("nan")):
        no(eng, INVALID, scale=scale)
    x = cu(lc.inputs("plain", 64, 128, 2))           # the handle still runs
    tp = _taps(eng, x)
    g = to_numpy(eng.attention_histograms_long_f32(x, 0, 0.5))
    ref = ahr.hist_f32(tp["logits"], tp["row_max"], tp["row_sum"], 0.5)
    assert all(np.array_equal(g[k], ref[k]) for k in NAMES)
