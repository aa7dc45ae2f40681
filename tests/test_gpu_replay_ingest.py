"""replay_frames(resize="gpu"): PNGs that are not 90 x 60 are uploaded at native size and depth and resized by Engine.ingest.  A
two-trajectory root of 120 x 180 PNGs, one 8-bit and one 16-bit: the replay equals, bit for bit, a frame-by-frame walk of
Engine.forward over ingest_reference of the decoded arrays; resize="pil" on the 8-bit trajectory still gives what it gave
(PIL's resize, the u8 wire path); a trajectory that mixes two non-native sizes is refused."""
import os

import numpy as np
import pytest

from conftest import golden_files
from drone_oa_iree_vit_accelerator_amd import host, params, replay, synth
from drone_oa_iree_vit_accelerator_amd.ingest_ref import ingest_reference

pytestmark = pytest.mark.gpu

HEADER = "idx,timestamp,desired_vel,quat_1,quat_2,quat_3,quat_4,pos_x,pos_y,pos_z,vel_x,vel_y,vel_z,extra\n"


def _make_root(tmp_path, specs, seed=0):
    """specs: per trajectory a list of (dtype, H, W) -> (root, {trajectory name: [decoded arrays]})"""
    from PIL import Image
    rs = np.random.RandomState(seed)
    root = tmp_path / "data"
    root.mkdir()
    arrays = {}
    for t, frames in enumerate(specs):
        name = f"traj_{t:02d}"
        d = root / name
        d.mkdir()
        rows, arrays[name] = [HEADER], []
        for k, (dt, H, W) in enumerate(frames):
            ts = 100.0 + t + 0.1 * k
            a = rs.randint(0, 65536 if dt == np.uint16 else 256, size=(H, W)).astype(dt)
            Image.fromarray(a).save(str(d / f"{ts:.3f}.png"))
            arrays[name].append(a)
            dv = float(rs.uniform(2, 8))
            q = rs.standard_normal(4)
            q /= np.linalg.norm(q)
            gt = rs.standard_normal(3)
            rows.append(f"{k},{ts + 0.0004:.4f},{dv:.6f},{q[0]:.6f},{q[1]:.6f},{q[2]:.6f},{q[3]:.6f},0,0,0,"
                        f"{gt[0]:.6f},{gt[1]:.6f},{gt[2]:.6f},x\n")
        (d / "data.csv").write_text("".join(rows))
    return root, arrays


@pytest.fixture(scope="module")
def engine():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    fx = params.load_fixture(golden_files("vitlstm_E64_seed0_B2.npz")[0])
    eng = host.Engine(params.blob_from_record(fx, synth.float_params(0, E=64), E=64), device=0, reserve=64)
    yield eng
    eng.close()


def _walk(engine, traj, frames_f32):
    """the reference's schedule: one frame per call from zero state, (h, c) carried -> [vel (3,)]"""
    import torch
    hidden, out = None, []
    for k, fr in enumerate(frames_f32):
        tel = traj.telemetry[k]
        dv = torch.tensor([tel.desired_velocity / 10.0], dtype=torch.float32, device="cuda")
        qt = torch.tensor([tel.quaternion], dtype=torch.float32, device="cuda")
        vel, hidden = engine.forward(torch.from_numpy(fr[None]).cuda(), dv, qt, hidden)
        out.append(vel.cpu().numpy()[0])
    return out


@pytest.mark.parametrize("schedule", ["steps", "sequence"])
def test_gpu_resize_equals_forward_on_the_reference_resize(tmp_path, engine, schedule):
    root, arrays = _make_root(tmp_path, [[(np.uint8, 120, 180)] * 3, [(np.uint16, 120, 180)] * 2])
    trajs = replay.scan_root(str(root))
    for t in trajs:                                   # the PNGs decode to what was written, 16 bits included
        for p, a in zip(t.frames, arrays[t.name]):
            got = replay.read_frame_native(p)
            assert got.dtype == a.dtype and (got == a).all()
    res = replay.replay_frames(engine, str(root), schedule=schedule, resize="gpu")
    assert engine.head_status() == 0
    assert [r.trajectory for r in res] == ["traj_00"] * 3 + ["traj_01"] * 2
    want = []
    for t in trajs:
        want += _walk(engine, t, ingest_reference(np.stack(arrays[t.name])))
    for r, w in zip(res, want):
        np.testing.assert_array_equal(r.output, w, err_msg=f"{r.trajectory}/{r.frame}")


def test_pil_resize_is_unchanged_and_is_the_default(tmp_path, engine):
    """today's result: PIL's bilinear resize on the host, then the u8 wire path, walked frame by frame"""
    import torch
    from PIL import Image
    root, arrays = _make_root(tmp_path, [[(np.uint8, 120, 180)] * 3])
    traj = replay.scan_root(str(root))[0]
    res = replay.replay(engine, str(root))
    again = replay.replay_frames(engine, str(root), resize="pil")
    hidden = None
    for k, (r, r2, a) in enumerate(zip(res, again, arrays["traj_00"])):
        small = np.asarray(Image.fromarray(a).resize((90, 60), Image.BILINEAR), dtype=np.uint8)
        tel = traj.telemetry[k]
        vel, hidden = engine.forward(torch.from_numpy(small[None]).cuda(),
                                     torch.tensor([tel.desired_velocity / 10.0], dtype=torch.float32, device="cuda"),
                                     torch.tensor([tel.quaternion], dtype=torch.float32, device="cuda"), hidden)
        np.testing.assert_array_equal(r.output, vel.cpu().numpy()[0])
        np.testing.assert_array_equal(r2.output, r.output)


@pytest.mark.parametrize("schedule", ["steps", "sequence"])
def test_wire_frames_stay_on_the_u8_path_beside_native_ones(tmp_path, engine, schedule):
    """resize="gpu" on a root whose first trajectory is 90 x 60 u8, in one group with a 120 x 180 one: the first one's
    results are those of replay() (the u8 wire path: the float32 path would differ in the last bits), whichever
    trajectories share its group, while the 120 x 180 one goes through ingest"""
    root, arrays = _make_root(tmp_path, [[(np.uint8, 60, 90)] * 2, [(np.uint8, 120, 180)] * 2])
    pil = replay.replay(engine, str(root), schedule=schedule)
    gpu = replay.replay_frames(engine, str(root), schedule=schedule, resize="gpu")
    assert engine.head_status() == 0
    assert [(r.trajectory, r.frame) for r in gpu] == [(r.trajectory, r.frame) for r in pil]
    for a, b in zip(pil[:2], gpu[:2]):
        np.testing.assert_array_equal(a.output, b.output)
    t1 = replay.scan_root(str(root))[1]
    for r, w in zip(gpu[2:], _walk(engine, t1, ingest_reference(np.stack(arrays["traj_01"])))):
        np.testing.assert_array_equal(r.output, w)


def test_a_trajectory_that_mixes_wire_and_native_frames(tmp_path, engine):
    """wire, native, native, wire, native in ONE trajectory (beside a wire-only and a native-only one): each frame on its
    own path with the state carried across, the same bits from both schedules and from a frame-by-frame walk"""
    import torch
    mixed = [(np.uint8, 60, 90), (np.uint16, 120, 180), (np.uint8, 120, 180), (np.uint8, 60, 90), (np.uint8, 120, 180)]
    root, arrays = _make_root(tmp_path, [mixed, [(np.uint8, 60, 90)] * 2, [(np.uint8, 120, 180)] * 3])
    steps = replay.replay_frames(engine, str(root), resize="gpu")
    seq = replay.replay_frames(engine, str(root), schedule="sequence", resize="gpu")
    assert engine.head_status() == 0
    assert [(r.trajectory, r.frame) for r in seq] == [(r.trajectory, r.frame) for r in steps] and len(steps) == 10
    for a, b in zip(steps, seq):
        np.testing.assert_array_equal(a.output, b.output, err_msg=f"{a.trajectory}/{a.frame}")
    traj, hidden = replay.scan_root(str(root))[0], None
    for k, a in enumerate(arrays["traj_00"]):
        img = torch.from_numpy(a[None].copy()).cuda() if a.shape == (60, 90) else torch.from_numpy(ingest_reference(a[None])).cuda()
        tel = traj.telemetry[k]
        vel, hidden = engine.forward(img, torch.tensor([tel.desired_velocity / 10.0], dtype=torch.float32, device="cuda"),
                                     torch.tensor([tel.quaternion], dtype=torch.float32, device="cuda"), hidden)
        np.testing.assert_array_equal(steps[k].output, vel.cpu().numpy()[0])


@pytest.mark.parametrize("schedule", ["steps", "sequence"])
def test_two_native_sizes_in_one_trajectory_are_refused(tmp_path, engine, schedule):
    root, _ = _make_root(tmp_path, [[(np.uint8, 120, 180), (np.uint8, 240, 320)]])
    with pytest.raises(ValueError, match="share one size"):
        replay.replay_frames(engine, str(root), schedule=schedule, resize="gpu")
    assert len(replay.replay(engine, str(root), schedule=schedule)) == 2          # the host resize takes them
