"""What one launch of a step stores for the next launch to read: the E = 64 encoder's x2 planes and the f32 token rows are
written through on per-frame buffer resources ("Write-through hand-overs"); the LSTM state and the planes
of ita_split_planes_kernel keep plain stores and are held to the same equalities.  Stores move the same bits, so everything
here is an equality: a wrong plane address, a lost half-row or a bad resource base moves a few rows of x2 and the velocities
by less than the oracle tolerance, and would hide behind the tolerance tests.

Each case is a few launches of at most 257 frames."""
import numpy as np
import pytest

from conftest import golden_files
from drone_oa_iree_vit_accelerator_amd import host, params, synth

pytestmark = pytest.mark.gpu

ORACLE_ATOL = 2e-5   # the bound of the forward tests against the CPU oracle (tests/test_gpu_parity.py, tail mode 1)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def e64(torch_cuda):
    """the seed-0 E = 64 model, 257 synthetic frames with their inputs and a random LSTM state, all on the GPU"""
    torch = torch_cuda
    d = params.load_fixture(golden_files("vitlstm_E64_seed0_B2.npz")[0])
    blob = params.blob_from_record(d, synth.float_params(0, E=64), E=64)
    fr = synth.frames(4100, 257)
    cu = lambda a: torch.from_numpy(a).cuda()
    state = [cu(np.random.RandomState(s).standard_normal((3, 257, 128)).astype(np.float32) * 0.1) for s in (11, 12)]
    return dict(blob=blob, fr=fr, img=cu(fr["img_u8"]), dv=cu(fr["desvel"]), qt=cu(fr["quat"]), h=state[0], c=state[1])


def _same(torch, got, want, what):
    for g, w, name in zip(got, want, ("vel", "h", "c")):
        assert torch.equal(g, w), f"{what}: {name} differs in {int((g != w).sum())} elements"


@pytest.mark.parametrize("B", [1, 33, 257], ids=["one_m_tile", "small_m_two_head_tiles", "tile128_partial_m"])
def test_planes_from_encoder_equal_planes_from_f32_rows(torch_cuda, e64, B):
    """forward writes the f16 hi / lo planes of x2 from the encoder kernel (and, asked for taps, the f32 rows beside them);
    ita_vitlstm_tail fed that f32 x2 splits it with ita_split_planes_kernel.  Same planes, same GEMM, same head: the three
    outputs are equal bit for bit.  B = 1: the one-M-tile GEMM; 33: the small-M GEMM and a second, partial 32-frame head tile;
    257: the 128 x 128 kernel with a partial M tile."""
    torch = torch_cuda
    eng = host.Engine(e64["blob"], device=0)
    hid = (e64["h"][:, :B].contiguous(), e64["c"][:, :B].contiguous())
    vel, (h, c), tp = eng.forward(e64["img"][:B], e64["dv"][:B], e64["qt"][:B], hid, taps=True)
    vel_t, (h_t, c_t) = eng.tail(tp["x2"], e64["dv"][:B], e64["qt"][:B], hid)
    _same(torch, (vel_t, h_t, c_t), (vel, h, c), f"tail from x2, B = {B}")
    # and the planes do not depend on whether the f32 rows were asked for
    vel_n, (h_n, c_n) = eng.forward(e64["img"][:B], e64["dv"][:B], e64["qt"][:B], hid)
    _same(torch, (vel_n, h_n, c_n), (vel, h, c), f"forward without taps, B = {B}")
    eng.close()


def test_state_in_place_and_slot_indexed_equal_out_of_place(torch_cuda, e64):
    """two consecutive steps at B = 33 (a whole and a partial head tile): h_out / c_out aliasing h_in / c_in, and the
    slot-indexed form with a permuted slot list over 40 state rows, against separate output tensors"""
    torch = torch_cuda
    B, NS = 33, 40
    eng = host.Engine(e64["blob"], device=0)
    steps = [(e64["img"][o:o + B], e64["dv"][o:o + B], e64["qt"][o:o + B]) for o in (0, 100)]
    h0, c0 = e64["h"][:, :B].contiguous(), e64["c"][:, :B].contiguous()
    want, hid = [], (h0, c0)
    for img, dv, qt in steps:
        vel, hid = eng.forward(img, dv, qt, hid)
        want.append((vel, hid[0], hid[1]))
    # in place
    hh, cc = h0.clone(), c0.clone()
    for t, (img, dv, qt) in enumerate(steps):
        vel = torch.empty((B, 3), dtype=torch.float32, device="cuda")
        eng.forward(img, dv, qt, (hh, cc), out=(vel, hh, cc))
        _same(torch, (vel, hh, cc), want[t], f"in place, step {t}")
    # slot-indexed, permuted
    slots = torch.from_numpy(np.random.RandomState(5).permutation(NS)[:B].astype(np.int32)).cuda()
    fill = torch.full((3, NS, 128), 7.0, dtype=torch.float32, device="cuda")
    sh, sc = fill.clone(), fill.clone()
    sh[:, slots.long()] = h0
    sc[:, slots.long()] = c0
    for t, (img, dv, qt) in enumerate(steps):
        vel = eng.forward_slots(img, dv, qt, sh, sc, slots)
        _same(torch, (vel, sh[:, slots.long()], sc[:, slots.long()]), want[t], f"slots, step {t}")
    rest = torch.ones(NS, dtype=torch.bool, device="cuda")
    rest[slots.long()] = False
    assert torch.equal(sh[:, rest], fill[:, rest]) and torch.equal(sc[:, rest], fill[:, rest]), "a row outside the slot list was written"
    eng.close()


def _frame_alone_equals_frame_in_batch(torch, oracle, blob, img_np, fr, what):
    B = img_np.shape[0]
    cu = lambda a: torch.from_numpy(a).cuda()
    eng = host.Engine(blob, device=0)
    img, dv, qt = cu(img_np), cu(fr["desvel"][:B]), cu(fr["quat"][:B])
    vel, (h, c) = eng.forward(img, dv, qt)
    for k in range(B):
        vk, (hk, ck) = eng.forward(img[k:k + 1], dv[k:k + 1], qt[k:k + 1])
        _same(torch, (vk, hk, ck), (vel[k:k + 1], h[:, k:k + 1], c[:, k:k + 1]), f"{what}: frame {k} alone")
    ov, oh, oc = oracle.forward(blob, img_np, fr["desvel"][:B], fr["quat"][:B])
    for got, ref, name in ((vel, ov, "vel"), (h, oh, "h"), (c, oc, "c")):
        np.testing.assert_allclose(got.cpu().numpy(), ref, atol=ORACLE_ATOL, rtol=0, err_msg=f"{what}: {name}")
    eng.close()


def test_token_rows_between_kernels_e128_two_layers(torch_cuda, oracle):
    """E = 128, two layers: the tokenizer launch and the first layer's kernels hand f32 token rows (64 KB per frame) to
    the next launch.  Frame k of a batch of five equals the same frame run alone, and the batch stays within the oracle bound."""
    d = params.load_fixture(golden_files("vit2l_*.npz")[0])
    nl = int(d["meta.num_layers"])
    fp = synth.float_params(int(d["meta.seed"]), E=128, num_layers=nl, tail=False)
    blob = params.blob_from_record(d, fp, E=128, num_layers=nl)
    fr = synth.frames(4200, 5)
    _frame_alone_equals_frame_in_batch(torch_cuda, oracle, blob, fr["img_u8"], fr, "vit2l")


def test_token_rows_between_kernels_e64_f32_frames(torch_cuda, oracle, e64):
    """E = 64 with f32 frames: the stand-alone tokenizer launch hands its rows to the encoder kernel without the fused tokenizer"""
    fr = synth.frames(4300, 5)
    img = fr["img_u8"].astype(np.float32) / np.float32(255.0)
    _frame_alone_equals_frame_in_batch(torch_cuda, oracle, e64["blob"], img, fr, "E = 64, f32 frames")


def test_sequence_equals_three_forward_calls(torch_cuda, e64):
    """T = 3 steps of ita_vitlstm_sequence at B = 33 against three forward calls: the head kernel and the sequence kernel store the
    state each in its own code and must agree bit for bit"""
    torch = torch_cuda
    T, B = 3, 33
    eng = host.Engine(e64["blob"], device=0, reserve=T * B)
    sl = [slice(o, o + B) for o in (0, 70, 140)]
    img = torch.stack([e64["img"][s] for s in sl])
    dv = torch.stack([e64["dv"][s] for s in sl])
    qt = torch.stack([e64["qt"][s] for s in sl])
    h0, c0 = e64["h"][:, :B].contiguous(), e64["c"][:, :B].contiguous()
    vel_s, (h_s, c_s) = eng.forward_sequence(img, dv, qt, (h0, c0))
    hid = (h0, c0)
    for t in range(T):
        vel, hid = eng.forward(img[t], dv[t], qt[t], hid)
        assert torch.equal(vel_s[t], vel), f"vel of step {t}"
    assert torch.equal(h_s, hid[0]) and torch.equal(c_s, hid[1])
    eng.close()
