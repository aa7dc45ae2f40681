"""Fusion tail on large token grids (BASELINE config 5).

CPU: the generalised oracle (oracle/ita_oracle.c:ita_oracle_tail_general) against outputs of the torch layers the
reference declares (tests/golden/tail_large_*.npz, tools/gen_golden.py:gen_tail_large): <= 2e-5 absolute (PyTorch's
conv summation order is not the oracle's), and its sampled form against the full form (equality); both, and the torch
outputs, against a float64 definition written from the layers alone (tail_common.tail_f64).
GPU (-m gpu): ita_fusion_tail_large through the C ABI against the oracle.  The kernel runs the convolution on
split-precision f16 MFMA (three products, f32 accumulate): tolerance 2e-5 relative to the largest output magnitude,
stated at the assertion (the task's bound for this tail is 1e-4).  Every kernel instantiation behind the call, the exact
cases, token magnitudes, refusals and reloads: test_gpu_tail_matrix.py.
"""
import numpy as np
import pytest

import tail_common as tc
from conftest import golden_files
from drone_oa_iree_vit_accelerator_amd import host, params, synth

FIX = golden_files("tail_large_*.npz")


def _case(path):
    d = params.load_fixture(path)
    meta = {k: int(d[k]) for k in ("seed", "E", "tok_h", "tok_w", "out_ch", "B")}
    c = synth.tail_large_case(meta["seed"], meta["E"], meta["tok_h"], meta["tok_w"], meta["out_ch"], meta["B"])
    assert synth.digest(c) == str(d["inputs_sha256"]), "synth.tail_large_case drifted from the committed fixture"
    return meta, c, d["out"]


def test_fixtures_present():
    assert len(FIX) >= 2


@pytest.mark.parametrize("path", FIX, ids=[p.split("/")[-1][:-4] for p in FIX])
def test_oracle_general_tail_vs_torch_layers(oracle, path):
    meta, c, want = _case(path)
    got = oracle.tail_general(c["x"], meta["tok_h"], meta["tok_w"], c["conv_w"], c["conv_b"])
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= 2e-5


def test_oracle_general_equals_model_tail(oracle):
    """on the model's own 8 x 16 grid with 9 outputs the general form IS ita_oracle_tail"""
    c = synth.tail_large_case(7, 64, 8, 16, 9, 2)
    a = oracle.tail_general(c["x"], 8, 16, c["conv_w"], c["conv_b"])
    b = oracle.tail(c["x"], c["conv_w"], c["conv_b"])
    assert np.array_equal(a.reshape(2, -1), b)


def test_oracle_sampled_equals_full(oracle):
    c = synth.tail_large_case(3, 128, 4, 16, 48, 2)
    full = oracle.tail_general(c["x"], 4, 16, c["conv_w"], c["conv_b"])
    rs = np.random.RandomState(0)
    pts = np.stack([rs.randint(0, 2, 300), rs.randint(0, 48, 300), rs.randint(0, 8, 300), rs.randint(0, 32, 300)], 1)
    pts[:8] = [[0, 0, 0, 0], [1, 47, 7, 31], [0, 5, 0, 31], [1, 9, 7, 0], [0, 1, 3, 0], [0, 2, 0, 5], [1, 3, 7, 9], [0, 4, 4, 31]]
    vals = oracle.tail_general_at(c["x"], 4, 16, c["conv_w"], c["conv_b"], pts.astype(np.int32))
    assert np.array_equal(vals, full[pts[:, 0], pts[:, 1], pts[:, 2], pts[:, 3]])


@pytest.mark.parametrize("path", FIX, ids=[p.split("/")[-1][:-4] for p in FIX])
def test_f64_definition_vs_torch_layers(path):
    """the float64 definition against what torch's own layers gave (f32: same bound as the oracle's comparison)"""
    meta, c, want = _case(path)
    got = tc.tail_f64(c["x"], meta["tok_h"], meta["tok_w"], c["conv_w"], c["conv_b"])
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= 2e-5


@pytest.mark.parametrize("shape", [(64, 4, 16, 9), (48, 8, 16, 33)], ids=tc.case_id)
def test_oracle_general_vs_f64_definition(oracle, shape):
    """The C oracle is one f32 fmaf chain of K = 9 * 5E/4 terms per output, over inputs that carry at most a few f32
    roundings of their own (the bilinear blend): its distance from the float64 definition is bounded by K 2^-24
    max|out| (the first-order bound of recursive f32 summation with a unit roundoff of 2^-24, in units of the largest
    output; derived, not tuned)."""
    E, th, tw, co = shape
    c = tc.case(shape)
    got = oracle.tail_general(c["x"], th, tw, c["conv_w"], c["conv_b"])
    want = tc.want_f64(shape)
    K = 9 * (5 * E // 4)
    err, bound = np.abs(got - want).max(), K * 2.0 ** -24 * np.abs(want).max()
    print(f"\n{tc.case_id(shape)}: max|oracle - f64| = {err:.3e}, bound {bound:.3e}")
    assert got.shape == want.shape and err <= bound


def test_matrix_reaches_every_kernel_variant():
    """tail_common.variant restates the dispatch of ita_fusion_tail_large; the GPU matrix and the exact cases name all nine"""
    assert {tc.variant(*s) for s in tc.MATRIX} == set(tc.VARIANTS)
    assert {tc.variant(*s) for s in tc.EXACT} == set(tc.VARIANTS)


@pytest.mark.parametrize("shape", tc.EXACT, ids=tc.case_id)
def test_integer_case_expectation_is_exact(shape):
    """the float64 result of the integer cases is integral and below 2^24: exactly representable in f32, and every
    partial sum of any summation order with it, so it is a zero-tolerance expectation for the kernels"""
    E, th, tw, co = shape
    c = tc.integer_case(shape, B=2)
    want = tc.tail_f64(c["x"], th, tw, c["conv_w"], c["conv_b"])
    assert np.array_equal(want, np.rint(want))
    # the largest partial sum any order can reach: sum |w| |x| + |b|, scaled as the loader scales the weights (max|w| = 4 -> 2^7)
    worst = 9 * (E // 4) * 4 * 8 * 128 + 16
    assert worst < 2 ** 24 and np.abs(want).max() <= worst
    assert np.all(c["conv_w"][:, E // 4:] == 0) and np.abs(c["conv_w"]).max() == 4 and np.abs(c["x"]).max() <= 8


# ------------------------------------------------------------------------------------------ GPU
def _run(torch, c, th, tw):
    eng = host.FusionTailLarge(c["conv_w"], c["conv_b"], device=0)
    out = eng(torch.from_numpy(c["x"]).cuda(), th, tw)
    torch.cuda.synchronize()
    res = out.cpu().numpy()
    eng.close()
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(128, 4, 16, 48, 2), (64, 8, 16, 9, 3), (128, 8, 32, 16, 1), (64, 4, 16, 33, 2),
                                   (128, 24, 48, 48, 1), (128, 16, 16, 20, 2), (64, 8, 16, 64, 2), (128, 8, 16, 64, 2)],
                         ids=["E128_4x16_co48", "E64_8x16_co9", "E128_8x32_co16", "E64_4x16_co33",
                              "E128_24x48_co48_interior_tiles", "E128_16x16_co20_one_tile_wide",
                              "E64_8x16_co64_16row_grid", "E128_8x16_co64_16row_grid"])
def test_gpu_tail_large_vs_oracle(oracle, shape):
    import torch
    E, th, tw, co, B = shape
    c = synth.tail_large_case(11, E, th, tw, co, B)
    want = oracle.tail_general(c["x"], th, tw, c["conv_w"], c["conv_b"])
    got = _run(torch, c, th, tw)
    assert got.shape == want.shape
    tol = 2e-5 * np.abs(want).max()      # f16x3 MFMA vs the f32 fmaf chain; task bound 1e-4
    assert np.abs(got - want).max() <= tol


@pytest.mark.gpu
@pytest.mark.parametrize("path", FIX, ids=[p.split("/")[-1][:-4] for p in FIX])
def test_gpu_tail_large_vs_golden(path):
    import torch
    meta, c, want = _case(path)
    got = _run(torch, c, meta["tok_h"], meta["tok_w"])
    assert np.abs(got - want).max() <= 4e-5 * max(1.0, np.abs(want).max())


@pytest.mark.gpu
def test_gpu_tail_config5_size(oracle):
    """BASELINE config 5's map (64 x 128 tokens, E = 128, 48 outputs; 2.26 G MAC per frame): sampled oracle
    comparison, run-to-run determinism, and independence of a frame's result from its batch position."""
    import torch
    E, th, tw, co, B = 128, 64, 128, 48, 2
    c = synth.tail_large_case(5, E, th, tw, co, B)
    eng = host.FusionTailLarge(c["conv_w"], c["conv_b"], device=0)
    x = torch.from_numpy(c["x"]).cuda()
    a = eng(x, th, tw)
    b = eng(x, th, tw)
    sw = eng(x.flip(0).contiguous(), th, tw)
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    assert torch.equal(a, sw.flip(0))
    got = a.cpu().numpy()
    rs = np.random.RandomState(1)
    n = 1500
    pts = np.stack([rs.randint(0, B, n), rs.randint(0, co, n), rs.randint(0, 2 * th, n), rs.randint(0, 2 * tw, n)], 1)
    pts[:6] = [[0, 0, 0, 0], [1, 47, 127, 255], [0, 7, 0, 255], [1, 8, 127, 0], [0, 20, 64, 128], [1, 33, 63, 31]]
    want = oracle.tail_general_at(c["x"], th, tw, c["conv_w"], c["conv_b"], pts.astype(np.int32))
    err = np.abs(got[pts[:, 0], pts[:, 1], pts[:, 2], pts[:, 3]] - want).max()
    assert err <= 2e-5 * max(1.0, np.abs(want).max())
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("B", [5, 32])
def test_gpu_tail_persistent_rounds(oracle, B):
    """More tiles than CUs: B frames of config 5's map are 64 B tiles for the 256 persistent workgroups of ita_tail_up_kernel
    (B = 5: 64 of them run a second tile, whose tokens they requested while finishing the first; B = 32: the bench's own
    launch, eight rounds).  A frame's map must not depend on the round or workgroup that produced it: frames equal the same
    frame run alone, bit for bit; and points sampled over the later rounds are checked against the oracle."""
    import torch
    E, th, tw, co = 128, 64, 128, 48
    c = synth.tail_large_case(9, E, th, tw, co, B)
    eng = host.FusionTailLarge(c["conv_w"], c["conv_b"], device=0)
    x = torch.from_numpy(c["x"]).cuda()
    full = eng(x, th, tw)
    for b in sorted({0, 3, 4, B // 2, B - 1}):
        alone = eng(x[b:b + 1].contiguous(), th, tw)
        assert torch.equal(full[b], alone[0]), f"frame {b}"
    rs = np.random.RandomState(2)
    n = 600
    pts = np.stack([rs.randint(4, B, n), rs.randint(0, co, n), rs.randint(0, 2 * th, n), rs.randint(0, 2 * tw, n)], 1)
    pts[:4] = [[B - 1, 0, 0, 0], [B - 1, 47, 127, 255], [4, 11, 0, 255], [4, 30, 127, 0]]
    got = full[torch.from_numpy(pts[:, 0]).cuda(), torch.from_numpy(pts[:, 1]).cuda(), torch.from_numpy(pts[:, 2]).cuda(),
               torch.from_numpy(pts[:, 3]).cuda()].cpu().numpy()
    want = oracle.tail_general_at(c["x"], th, tw, c["conv_w"], c["conv_b"], pts.astype(np.int32))
    err = np.abs(got - want).max()
    assert err <= 2e-5 * max(1.0, np.abs(want).max())
    eng.close()


@pytest.mark.gpu
def test_gpu_tail_large_rejects_bad_shapes():
    import torch
    c = synth.tail_large_case(0, 64, 4, 16, 9, 1)
    eng = host.FusionTailLarge(c["conv_w"], c["conv_b"], device=0)
    with pytest.raises(host.ITAError):
        eng(torch.zeros((1, 3 * 16, 64), device="cuda"), 3, 16)      # tok_h % 4
    with pytest.raises(host.ITAError):
        eng(torch.zeros((1, 4 * 8, 64), device="cuda"), 4, 8)        # tok_w % 16
    eng.close()
