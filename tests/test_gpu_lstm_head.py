"""The LSTM head of tail mode 1 (ita_lstm_head_kernel: layers 0, 1, 2 and the fc in one launch whose workgroups meet
twice per 32-frame tile): a frame's result does not depend on the batch it runs in, on a grid larger than the GPU holds
at once, under graph replay or next to another stream's work.  After every call the head's device error word is 0."""
import os

import numpy as np
import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu


def _engine():
    from drone_oa_iree_vit_accelerator_amd import host, params, synth
    fx = params.load_fixture(os.path.join(REPO, "tests", "golden", "vitlstm_E64_seed0_B2.npz"))
    blob = params.blob_from_record(fx, synth.float_params(0, E=64), E=64)
    return host.Engine(blob, device=0), blob


def _inputs(seed, B):
    from drone_oa_iree_vit_accelerator_amd import synth
    fr = synth.frames(seed, B)
    rs = np.random.RandomState(seed)
    h0 = (0.3 * rs.standard_normal((3, B, 128))).astype(np.float32)
    c0 = (0.3 * rs.standard_normal((3, B, 128))).astype(np.float32)
    return fr["img_u8"], fr["desvel"], fr["quat"], h0, c0


def _forward(eng, img, dv, qt, h0, c0):
    import torch
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    vel, (h, c) = eng.forward(cu(img), cu(dv), cu(qt), (cu(h0), cu(c0)))
    torch.cuda.synchronize()
    assert eng.head_status() == 0
    return vel.cpu().numpy(), h.cpu().numpy(), c.cpu().numpy()


def test_frames_independent_of_batch():
    """each frame's vel / h / c equals, bit for bit, the same frame inside a 1024-frame batch: B = 1 and 31 (one partial
    frame tile), 32 (one whole tile), 33 (a tile of one frame), 1000 (a partial last tile)"""
    eng, _ = _engine()
    img, dv, qt, h0, c0 = _inputs(7, 1024)
    ref = _forward(eng, img, dv, qt, h0, c0)
    for B, at in ((1, 517), (31, 3), (32, 64), (33, 990 - 33), (1000, 24)):
        sl = slice(at, at + B)
        got = _forward(eng, img[sl], dv[sl], qt[sl], h0[:, sl], c0[:, sl])
        np.testing.assert_array_equal(got[0], ref[0][sl], err_msg=f"vel B={B}")
        np.testing.assert_array_equal(got[1], ref[1][:, sl], err_msg=f"h B={B}")
        np.testing.assert_array_equal(got[2], ref[2][:, sl], err_msg=f"c B={B}")
    eng.close()


def test_grid_larger_than_resident(oracle):
    """The kernel holds two 256-thread workgroups per CU (246 VGPRs -> 2 waves per SIMD, 54 KB of LDS), so the GPU holds
    2 * CUs workgroups at once: 512 on an MI355X, i.e. 1024 frames.  A batch of 8 * CUs + 7 frames (2055 on an MI355X)
    launches 16 * ceil(B / 32) >= 4 * CUs workgroups, twice what is resident.  Sampled frames, from the first and the last
    tiles as well, meet the oracle within 2e-5 and equal the same frames run as a small batch bit for bit."""
    import torch
    eng, blob = _engine()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B = 8 * cus + 7
    assert 16 * ((B + 31) // 32) >= 2 * (2 * cus)
    img, dv, qt, h0, c0 = _inputs(11, B)
    vel, h, c = _forward(eng, img, dv, qt, h0, c0)
    pick = np.array([0, 31, 32, 777, B // 2, B - 33, B - 2, B - 1])
    ovel, oh, oc = oracle.forward(blob, img[pick], dv[pick], qt[pick], h0[:, pick], c0[:, pick])
    for name, g, o in (("vel", vel[pick], ovel), ("h", h[:, pick], oh), ("c", c[:, pick], oc)):
        err = float(np.abs(g - o).max())
        print(f"B={B}: {name} max|gpu - oracle| = {err:.3e}")
        assert err <= 2e-5, name
    small = _forward(eng, img[pick], dv[pick], qt[pick], h0[:, pick], c0[:, pick])
    np.testing.assert_array_equal(small[0], vel[pick])
    np.testing.assert_array_equal(small[1], h[:, pick])
    np.testing.assert_array_equal(small[2], c[:, pick])
    eng.close()


def _sequential(eng, frames, B, n):
    """n forwards on one stream from zero state, frames[t % len(frames)] at step t"""
    import torch
    st = None
    for t in range(n):
        img, dv, qt = frames[t % len(frames)]
        v, st = eng.forward(img, dv, qt, st)
    torch.cuda.synchronize()
    assert eng.head_status() == 0
    return v.cpu().numpy(), st[0].cpu().numpy(), st[1].cpu().numpy()


def _frames(B):
    import torch
    from drone_oa_iree_vit_accelerator_amd import synth
    out = []
    for s in range(4):
        fr = synth.frames(40 + s, B)
        out.append(tuple(torch.from_numpy(fr[k]).cuda() for k in ("img_u8", "desvel", "quat")))
    return out


@pytest.mark.parametrize("B", [96, 1024])
def test_graph_replay_equals_sequential(B):
    """64 replays of the captured step (the head's counters are re-armed in-kernel, replay after replay) equal 64
    sequential single-stream forwards bit for bit"""
    eng, _ = _engine()
    frames = _frames(B)
    ref = _sequential(eng, frames, B, 64)
    g = eng.graphed_step(B)
    for t in range(64):
        img, dv, qt = frames[t % len(frames)]
        g.img.copy_(img); g.desvel.copy_(dv.reshape(-1)); g.quat.copy_(qt.reshape(-1, 4))
        g()
    import torch
    torch.cuda.synchronize()
    assert eng.head_status() == 0
    np.testing.assert_array_equal(g.vel.cpu().numpy(), ref[0])
    np.testing.assert_array_equal(g.h.cpu().numpy(), ref[1])
    np.testing.assert_array_equal(g.c.cpu().numpy(), ref[2])
    eng.close()


def test_steps_beside_a_busy_stream_equal_sequential():
    """64 steps while a second stream keeps the GPU busy with long GEMMs (so the head's workgroups are dispatched as CUs
    free up, not all at once) equal 64 sequential forwards on an idle GPU bit for bit"""
    import torch
    B = 1024
    eng, _ = _engine()
    frames = _frames(B)
    ref = _sequential(eng, frames, B, 64)
    busy = torch.cuda.Stream()
    a = torch.randn(4096, 4096, device="cuda")
    st = None
    for t in range(64):
        with torch.cuda.stream(busy):
            for _ in range(2):
                a = torch.tanh(a @ a * 1e-3)
        img, dv, qt = frames[t % len(frames)]
        v, st = eng.forward(img, dv, qt, st)
    torch.cuda.synchronize()
    assert eng.head_status() == 0
    np.testing.assert_array_equal(v.cpu().numpy(), ref[0])
    np.testing.assert_array_equal(st[0].cpu().numpy(), ref[1])
    np.testing.assert_array_equal(st[1].cpu().numpy(), ref[2])
    eng.close()
