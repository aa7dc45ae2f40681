"""The folded GEMM's three kernels (tiny: <= 32 frames, small: 33..256, large: above) share one per-element arithmetic --
k-steps of 32, three split-precision products per step on v_mfma_f32_16x16x32_f16 with the weights as the A operand, 16-byte
partial stores -- so a frame's result must not depend on which of them served its batch.

Batch sizes and the kernel each reaches (launch_gemm_split):
    5    tiny, one 16-frame MFMA tile
    20   tiny, two 16-frame MFMA tiles
    33   small, MT = 2, ragged second M tile
    130  small, MT = 4, a second row of workgroups holding 2 frames
    257  large, the last 128-row tile holds 1 frame
Against the oracle the folded path keeps the bound tests/test_gpu_parity.py uses for it: 2e-5 absolute on vel, h and c."""
import numpy as np
import pytest

from conftest import golden_files
from drone_oa_iree_vit_accelerator_amd import host, params, synth

pytestmark = pytest.mark.gpu

BATCHES = (5, 20, 33, 130, 257)
FOLDED_TOL = dict(atol=2e-5, rtol=0)   # tests/test_gpu_parity.py: the folded (f16x3) path against the oracle


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _inputs(torch, seed, B):
    fr = synth.frames(seed, B)
    cu = lambda a: torch.from_numpy(a).cuda()
    h = np.random.RandomState(seed + 1).standard_normal((3, B, 128)).astype(np.float32) * 0.1
    c = np.random.RandomState(seed + 2).standard_normal((3, B, 128)).astype(np.float32) * 0.1
    return fr, h, c, (cu(fr["img_u8"]), cu(fr["desvel"]), cu(fr["quat"]), cu(h), cu(c))


def _run(eng, dev, n=None, idx=None):
    img, dv, qt, h, c = dev
    if idx is None:
        idx = slice(0, n)
    v, (ho, co) = eng.forward(img[idx], dv[idx], qt[idx], (h[:, idx].contiguous(), c[:, idx].contiguous()))
    return v, ho, co


@pytest.fixture(scope="module")
def e64(torch_cuda):
    """E = 64 seed-0 blob, u8 frames: one forward per batch size, shared by the tests below (and left unchanged)"""
    d = params.load_fixture(golden_files("vitlstm_E64_seed0_B2.npz")[0])
    blob = params.blob_from_record(d, synth.float_params(0, E=64), E=64)
    eng = host.Engine(blob, device=0)
    fr, h, c, dev = _inputs(torch_cuda, 91, 257)
    runs = {n: _run(eng, dev, n) for n in BATCHES}
    yield dict(eng=eng, blob=blob, fr=fr, h=h, c=c, dev=dev, runs=runs)
    eng.close()


def test_batch_composition_independence_e64(torch_cuda, e64):
    torch = torch_cuda
    ref = e64["runs"][5]
    for n in BATCHES[1:]:
        v, h, c = e64["runs"][n]
        assert torch.equal(v[:5], ref[0]) and torch.equal(h[:, :5], ref[1]) and torch.equal(c[:, :5], ref[2]), n
    # frame 256 (alone in the large kernel's last 128-row tile) against the same frame in a batch of 5 (tiny kernel)
    idx = torch.tensor([256, 1, 2, 3, 4], device="cuda")
    vs, hs, cs = _run(e64["eng"], e64["dev"], idx=idx)
    v, h, c = e64["runs"][257]
    assert torch.equal(vs[0], v[256]) and torch.equal(hs[:, 0], h[:, 256]) and torch.equal(cs[:, 0], c[:, 256])


def test_batch_composition_independence_e128_two_layers(torch_cuda):
    """the two-layer E = 128 graph: K = 16384, 32 k-tiles per slice"""
    torch = torch_cuda
    d = params.load_fixture(golden_files("vit2l_*.npz")[0])
    nl = int(d["meta.num_layers"])
    blob = params.blob_from_record(d, synth.float_params(int(d["meta.seed"]), E=128, num_layers=nl, tail=False), E=128, num_layers=nl)
    eng = host.Engine(blob, device=0)
    _, _, _, dev = _inputs(torch, 92, 257)
    v5, h5, c5 = _run(eng, dev, 5)
    v, h, c = _run(eng, dev, 257)
    assert torch.equal(v[:5], v5) and torch.equal(h[:, :5], h5) and torch.equal(c[:, :5], c5)
    idx = torch.tensor([256, 1, 2, 3, 4], device="cuda")
    vs, hs, cs = _run(eng, dev, idx=idx)
    assert torch.equal(vs[0], v[256]) and torch.equal(hs[:, 0], h[:, 256]) and torch.equal(cs[:, 0], c[:, 256])
    eng.close()


def test_against_oracle(e64, oracle):
    sel = [0, 1, 2, 3, 127, 128, 255, 256]
    fr = e64["fr"]
    ov, oh, oc = oracle.forward(e64["blob"], fr["img_u8"][sel], fr["desvel"][sel], fr["quat"][sel], e64["h"][:, sel], e64["c"][:, sel])
    v, h, c = e64["runs"][257]
    np.testing.assert_allclose(v.cpu().numpy()[sel], ov, **FOLDED_TOL)
    np.testing.assert_allclose(h.cpu().numpy()[:, sel], oh, **FOLDED_TOL)
    np.testing.assert_allclose(c.cpu().numpy()[:, sel], oc, **FOLDED_TOL)


def test_determinism(torch_cuda, e64):
    torch = torch_cuda
    v, h, c = e64["runs"][257]
    v2, h2, c2 = _run(e64["eng"], e64["dev"], 257)
    assert torch.equal(v, v2) and torch.equal(h, h2) and torch.equal(c, c2)
