"""Engine.forward_sequence (ita_vitlstm_sequence: the image-only part of T steps x B streams as one batch of T * B frames,
the recurrence as one ita_lstm_seq_kernel launch per chunk) against the step path: T calls of Engine.forward, which it has
to equal bit for bit -- across chunk seams, partial stream tiles, per-stream lengths, in place, on a grid larger than the
GPU holds at once, interleaved with the step path's own head kernel, and for every blob family the front serves.  After
every call the head's device error word is 0.

A launch of the kernel runs Tc = workspace frames / B steps, and an engine that was never reserved holds only the largest
batch it has seen (Tc = 1).  So every test that is about the time loop reserves T * B frames first and checks, through
_whole(), that its T steps are ONE launch; the one-step-per-launch form is kept as a variant of its own."""
import os

import numpy as np
import pytest

from conftest import REPO, golden_files
from gpu_support import cu

pytestmark = pytest.mark.gpu


def _blob():
    from drone_oa_iree_vit_accelerator_amd import params, synth
    fx = params.load_fixture(os.path.join(REPO, "tests", "golden", "vitlstm_E64_seed0_B2.npz"))
    return params.blob_from_record(fx, synth.float_params(0, E=64), E=64)


def _engine(reserve=0):
    from drone_oa_iree_vit_accelerator_amd import host
    blob = _blob()
    return host.Engine(blob, device=0, reserve=reserve), blob


def _whole(eng, T, B):
    """the engine's workspace is pinned for at least T * B frames: T steps of B streams are one launch of T steps"""
    assert eng._reserved // B >= T, f"workspace of {eng._reserved} frames: {eng._reserved // B} steps per launch, wanted {T}"


def _inputs(seed, T, B, zero_state=False):
    """time-major u8 frames, desvel, quat of T steps x B streams and a non-zero initial state"""
    from drone_oa_iree_vit_accelerator_amd import synth
    fr = synth.frames(seed, T * B)
    rs = np.random.RandomState(seed)
    h0 = (0.3 * rs.standard_normal((3, B, 128))).astype(np.float32)
    c0 = (0.3 * rs.standard_normal((3, B, 128))).astype(np.float32)
    if zero_state:
        h0[:], c0[:] = 0, 0
    return (fr["img_u8"].reshape(T, B, 60, 90), fr["desvel"].reshape(T, B).astype(np.float32),
            fr["quat"].reshape(T, B, 4).astype(np.float32), h0, c0)


def _steps(eng, img, dv, qt, h0, c0, T=None):
    """the reference: T calls of Engine.forward, state carried -> (vel (T,B,3), h, c)"""
    import torch
    T = img.shape[0] if T is None else T
    st = (cu(h0), cu(c0))
    vels = []
    for t in range(T):
        v, st = eng.forward(cu(img[t]), cu(dv[t]), cu(qt[t]), st)
        vels.append(v)
    torch.cuda.synchronize()
    assert eng.head_status() == 0
    B = img.shape[1]
    vel = torch.stack(vels).cpu().numpy() if vels else np.zeros((0, B, 3), np.float32)
    return vel, st[0].cpu().numpy(), st[1].cpu().numpy()


def _sequence(eng, img, dv, qt, h0, c0, **kw):
    import torch
    vel, (h, c) = eng.forward_sequence(cu(img), cu(dv), cu(qt), (cu(h0), cu(c0)), **kw)
    torch.cuda.synchronize()
    assert eng.head_status() == 0
    return vel.cpu().numpy(), h.cpu().numpy(), c.cpu().numpy()


def _assert_equal(got, ref, what=""):
    for name, g, r in zip(("vel", "h", "c"), got, ref):
        np.testing.assert_array_equal(g, r, err_msg=f"{what} {name}")


@pytest.mark.parametrize("T,B", [(1, 1), (3, 1), (64, 1), (17, 5), (9, 32), (6, 33), (5, 100), (3, 1000)])
def test_equals_step_path(T, B):
    """all T steps in ONE launch (workspace reserved for T * B frames): one partial tile, one whole tile, a tile of one
    stream, four tiles (5, 100) and 32 tiles -- 512 workgroups, twice what is resident -- (3, 1000)"""
    eng, _ = _engine(reserve=T * B)
    _whole(eng, T, B)
    x = _inputs(100 + T + B, T, B)
    ref = _steps(eng, *x)
    _assert_equal(_sequence(eng, *x), ref, f"T={T} B={B}")
    eng.close()


@pytest.mark.parametrize("T,B", [(3, 1), (17, 5), (6, 33), (3, 1000)])
def test_equals_step_path_one_step_per_launch(T, B):
    """an engine that was never reserved holds B frames after the reference's first step: T launches of ONE step each
    (initial-state meeting, one pass of the loop, the end), the state carried through memory from launch to launch"""
    eng, _ = _engine()
    x = _inputs(100 + T + B, T, B)
    ref = _steps(eng, *x)
    assert eng._reserved == 0
    _assert_equal(_sequence(eng, *x), ref, f"T={T} B={B}")
    eng.close()


@pytest.mark.parametrize("T,B", [(300, 3), (3, 1000)])
def test_equals_step_path_across_chunk_seams(T, B):
    """workspace pinned at 256 frames: (300, 3) runs in chunks of 85 steps, (3, 1000) has more streams than the workspace
    holds frames (one step per launch, after a new reserve)"""
    eng, _ = _engine(reserve=256)
    if B > 256:
        eng.reserve(B)
    x = _inputs(7 + T, T, B)
    ref = _steps(eng, *x)
    _assert_equal(_sequence(eng, *x), ref, f"T={T} B={B}")
    eng.close()


@pytest.mark.parametrize("T,B", [(300, 3), (40, 64)])
def test_many_chunks_and_lengths(T, B):
    """workspace pinned at 256 frames: (300, 3) is launches of 85, 85, 85, 45 steps; (40, 64) is ten launches of 4 steps,
    with per-stream lengths that end inside, at and behind chunk seams"""
    import torch
    eng, _ = _engine(reserve=256)
    img, dv, qt, h0, c0 = _inputs(50 + T, T, B)
    ref = _steps(eng, img, dv, qt, h0, c0)
    _assert_equal(_sequence(eng, img, dv, qt, h0, c0), ref, f"T={T} B={B}")
    if B == 64:
        # the second stream tile is finished after five steps: in later chunks its workgroups have nothing to do
        lens = np.array([T, 0, 1, 4, 5, 17, 36, 39] * 4 + [3, 0, 1, 4, 5, 2, 4, 5] * 4, np.int32)
        vel, h, c = _sequence(eng, img, dv, qt, h0, c0, lengths=torch.from_numpy(lens))
        for b in (0, 1, 2, 3, 4, 13, 31, 32, 36, 62, 63):
            sl = slice(b, b + 1)
            rv, rh, rc = _steps(eng, img[:, sl], dv[:, sl], qt[:, sl], h0[:, sl], c0[:, sl], T=int(lens[b]))
            np.testing.assert_array_equal(vel[:lens[b], b], rv[:, 0], err_msg=f"vel stream {b}")
            np.testing.assert_array_equal(h[:, b], rh[:, 0], err_msg=f"h stream {b}")
            np.testing.assert_array_equal(c[:, b], rc[:, 0], err_msg=f"c stream {b}")
    eng.close()


def test_f32_frames():
    """one launch of 8 steps"""
    T, B = 8, 4
    eng, _ = _engine(reserve=T * B)
    _whole(eng, T, B)
    img, dv, qt, h0, c0 = _inputs(21, T, B)
    imgf = img.astype(np.float32) / 255.0
    ref = _steps(eng, imgf, dv, qt, h0, c0)
    _assert_equal(_sequence(eng, imgf, dv, qt, h0, c0), ref, "f32")
    eng.close()


def test_lengths():
    """each stream's valid rows and final state equal that stream run alone through the step path for its own length; a
    stream of length 0 keeps its state; rows behind a stream's length keep what the caller had in `out`.  One launch of
    12 steps: streams freeze inside the time loop, at steps 7, 1 and 0."""
    import torch
    T, B = 12, 5
    eng, _ = _engine(reserve=T * B)
    _whole(eng, T, B)
    lens = [12, 7, 1, 0, 12]
    img, dv, qt, h0, c0 = _inputs(33, T, B)
    vel = torch.full((T, B, 3), -77.0, device="cuda")
    h, c = cu(h0), cu(c0)
    hin, cin = h.clone(), c.clone()
    out = eng.forward_sequence(cu(img), cu(dv), cu(qt), (hin, cin), lengths=torch.tensor(lens), out=(vel, h, c))
    torch.cuda.synchronize()
    assert eng.head_status() == 0
    assert out[0] is vel and out[1][0] is h and out[1][1] is c
    vel, h, c = vel.cpu().numpy(), h.cpu().numpy(), c.cpu().numpy()
    for b, n in enumerate(lens):
        sl = slice(b, b + 1)
        rv, rh, rc = _steps(eng, img[:, sl], dv[:, sl], qt[:, sl], h0[:, sl], c0[:, sl], T=n)
        np.testing.assert_array_equal(vel[:n, b], rv[:, 0], err_msg=f"vel stream {b}")
        np.testing.assert_array_equal(h[:, b], rh[:, 0], err_msg=f"h stream {b}")
        np.testing.assert_array_equal(c[:, b], rc[:, 0], err_msg=f"c stream {b}")
        assert (vel[n:, b] == -77.0).all(), f"stream {b}: rows behind its length were written"
    np.testing.assert_array_equal(h[:, 3], h0[:, 3])
    np.testing.assert_array_equal(c[:, 3], c0[:, 3])
    eng.close()


@pytest.mark.parametrize("T,B", [(10, 40), (7, 200)])
def test_in_place(T, B):
    """one launch of T steps on two / seven stream tiles, the state tensors handed in and back"""
    import torch
    eng, _ = _engine(reserve=T * B)
    _whole(eng, T, B)
    img, dv, qt, h0, c0 = _inputs(5, T, B)
    ref = _sequence(eng, img, dv, qt, h0, c0)
    h, c = cu(h0), cu(c0)
    vel = torch.empty((T, B, 3), device="cuda")
    eng.forward_sequence(cu(img), cu(dv), cu(qt), (h, c), out=(vel, h, c))
    torch.cuda.synchronize()
    assert eng.head_status() == 0
    _assert_equal((vel.cpu().numpy(), h.cpu().numpy(), c.cpu().numpy()), ref, "in place")
    _assert_equal(ref, _steps(eng, img, dv, qt, h0, c0), "out of place")
    eng.close()


def test_hidden_not_modified():
    """one launch of 3 steps"""
    import torch
    eng, _ = _engine(reserve=6)
    _whole(eng, 3, 2)
    img, dv, qt, h0, c0 = _inputs(6, 3, 2)
    h, c = cu(h0), cu(c0)
    eng.forward_sequence(cu(img), cu(dv), cu(qt), (h, c))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(h.cpu().numpy(), h0)
    np.testing.assert_array_equal(c.cpu().numpy(), c0)
    eng.close()


def test_oracle(oracle):
    """the bound tests/test_replay.py::test_replay_trajectory_equals_oracle holds the step path's velocities to over four
    steps; h and c at the same 2e-5, as tests/test_gpu_lstm_head.py::test_grid_larger_than_resident holds the head's.
    One launch of 4 steps."""
    T, B = 4, 2
    eng, blob = _engine(reserve=T * B)
    _whole(eng, T, B)
    img, dv, qt, h0, c0 = _inputs(44, T, B, zero_state=True)
    vel, h, c = _sequence(eng, img, dv, qt, h0, c0)
    oh = oc = None
    for t in range(T):
        ov, oh, oc = oracle.forward(blob, img[t], dv[t], qt[t], oh, oc)
        err = float(np.abs(vel[t] - ov).max())
        print(f"step {t}: max|vel - oracle| = {err:.3e}")
        np.testing.assert_allclose(vel[t], ov, atol=2e-5, rtol=0, err_msg=f"step {t}")
    np.testing.assert_allclose(h, oh, atol=2e-5, rtol=0)
    np.testing.assert_allclose(c, oc, atol=2e-5, rtol=0)
    eng.close()


def test_grid_larger_than_resident():
    """B = 8 * CUs + 7 streams launch 16 * ceil(B / 32) >= 4 * CUs workgroups of a kernel of which a CU holds one: four
    times what is resident, in ONE launch of 3 steps (workspace reserved for 3 * B frames): the tiles run in rounds with the
    time loop going.  Sampled streams from the first, a middle and the last tile equal the same streams run as a small batch
    through the step path, bit for bit."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    T, B = 3, 8 * cus + 7
    eng, _ = _engine(reserve=T * B)
    _whole(eng, T, B)
    assert 16 * ((B + 31) // 32) >= 2 * (2 * cus)
    img, dv, qt, h0, c0 = _inputs(11, T, B)
    vel, h, c = _sequence(eng, img, dv, qt, h0, c0)
    pick = np.array([0, 31, 32, 777, B // 2, B - 33, B - 2, B - 1])
    ref = _steps(eng, img[:, pick], dv[:, pick], qt[:, pick], h0[:, pick], c0[:, pick])
    _assert_equal((vel[:, pick], h[:, pick], c[:, pick]), ref, f"B={B}")
    eng.close()


def test_interleaved_with_the_step_path():
    """forward, forward_sequence (one launch of 5 steps), graph replays of the step, forward_sequence on one engine: each
    equals its own reference, so every launch found the arrival counters at 0"""
    import torch
    from drone_oa_iree_vit_accelerator_amd import host
    blob = _blob()
    B, T = 40, 5
    ref_eng = host.Engine(blob, device=0)
    x1 = _inputs(71, 1, B)
    x2 = _inputs(72, T, B)
    x3 = _inputs(73, 3, B, zero_state=True)
    x4 = _inputs(74, T, B)
    r1, r2, r3, r4 = (_steps(ref_eng, *x) for x in (x1, x2, x3, x4))
    ref_eng.close()
    eng = host.Engine(blob, device=0, reserve=T * B)
    _whole(eng, T, B)
    _assert_equal(_steps(eng, *x1), r1, "forward")
    _assert_equal(_sequence(eng, *x2), r2, "sequence 1")
    g = eng.graphed_step(B)
    for t in range(3):
        g.img.copy_(cu(x3[0][t])); g.desvel.copy_(cu(x3[1][t])); g.quat.copy_(cu(x3[2][t]))
        g()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(g.vel.cpu().numpy(), r3[0][t], err_msg=f"graph step {t}")
    assert eng.head_status() == 0
    np.testing.assert_array_equal(g.h.cpu().numpy(), r3[1])
    np.testing.assert_array_equal(g.c.cpu().numpy(), r3[2])
    _assert_equal(_sequence(eng, *x4), r4, "sequence 2")
    del g
    eng.close()


def _family_blob(family):
    from drone_oa_iree_vit_accelerator_amd import params, synth
    if family == "qat_e128_2l_no_tail":      # tests/test_gpu_parity.py::test_two_layer_e128_no_tail_graph
        d = params.load_fixture(golden_files("vit2l_E128_s0_B2.npz")[0])
        nl = int(d["meta.num_layers"])
        fp = synth.float_params(int(d["meta.seed"]), E=128, num_layers=nl, tail=False)
        return params.blob_from_record(d, fp, E=128, num_layers=nl)
    if family == "itaw0002":                 # tests/test_gpu_only_attn.py
        d = params.load_fixture(golden_files("onlyattn1l_E64_s0_B2.npz")[0])
        fp = synth.float_params(int(d["meta.seed"]), E=64, num_layers=int(d["meta.num_layers"]))
        return params.blob_from_record(d, fp, E=64, num_layers=1)
    if family == "itaw0003_e64":             # tests/test_gpu_float_graph.py
        d = params.load_fixture(golden_files("floattwin_E64_s0_B2.npz")[0])
        return params.blob_from_float_params(synth.float_params(int(d["meta.seed"]), E=64, num_layers=1), 1)
    d = params.load_fixture(golden_files("floatnt2l_E128_s1_B2.npz")[0])   # tests/test_gpu_float_e128.py
    return params.blob_from_float_params(synth.float_params(int(d["meta.seed"]), E=128, num_layers=2, tail=False), 2)


@pytest.mark.parametrize("family", ["qat_e128_2l_no_tail", "itaw0002", "itaw0003_e64", "itaw0003_e128"])
def test_other_blob_families(family):
    """one launch of 6 steps (workspace reserved for the 18 frames)"""
    from drone_oa_iree_vit_accelerator_amd import host
    T, B = 6, 3
    eng = host.Engine(_family_blob(family), device=0, reserve=T * B)
    _whole(eng, T, B)
    img, dv, qt, h0, c0 = _inputs(90, T, B)
    # premise, on the step path alone: this family's front does not depend on the batch a frame runs in.  A failure HERE is
    # a finding about the existing path, not about forward_sequence.
    flat = lambda a, n: np.ascontiguousarray(a.reshape((T * B,) + a.shape[2:])[:n])
    hh, cc = np.tile(h0, (1, T, 1)), np.tile(c0, (1, T, 1))
    big = _steps(eng, flat(img, 18)[None], flat(dv, 18)[None], flat(qt, 18)[None], hh, cc)
    small = _steps(eng, flat(img, 3)[None], flat(dv, 3)[None], flat(qt, 3)[None], hh[:, :3], cc[:, :3])
    _assert_equal((big[0][:, :3], big[1][:, :3], big[2][:, :3]), small, f"{family}: step path, batch 18 against batch 3:")
    ref = _steps(eng, img, dv, qt, h0, c0)
    _assert_equal(_sequence(eng, img, dv, qt, h0, c0), ref, family)
    eng.close()


def test_tail_mode_0_is_refused():
    import torch
    from drone_oa_iree_vit_accelerator_amd import host
    eng, _ = _engine()
    eng.set_tail_mode(0)
    img, dv, qt, h0, c0 = _inputs(3, 2, 2)
    vel = torch.full((2, 2, 3), -5.0, device="cuda")
    h, c = cu(h0), cu(c0)
    with pytest.raises(host.ITAError) as ei:
        eng.forward_sequence(cu(img), cu(dv), cu(qt), (h, c), out=(vel, h, c))
    assert str(ei.value).startswith("ita status -4:")   # ITA_ERR_UNSUPPORTED
    assert host.lib().ita_last_error() == -4
    torch.cuda.synchronize()
    assert (vel.cpu().numpy() == -5.0).all()           # nothing was launched
    np.testing.assert_array_equal(h.cpu().numpy(), h0)
    eng.close()
