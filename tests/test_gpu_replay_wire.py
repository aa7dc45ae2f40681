"""replay_frames(resize="stb"): PNGs that are not 90 x 60 are read as 8 bits, uploaded at native size, resized by
Engine.ingest_wire with the reference host's stb filters and run as u8 wire frames.  Two short synthetic trajectories of
96 x 128 8-bit PNGs (and a 16-bit one, converted as stbi_load(..., 1) converts it): for both schedules the replay equals,
bit for bit, a frame-by-frame walk of Engine.forward over the definition's codes, and the per-frame CPU oracle on those
codes within the bound tests/test_replay.py holds the step path to."""
import numpy as np
import pytest

from conftest import golden_files
from drone_oa_iree_vit_accelerator_amd import host, params, replay, synth
from drone_oa_iree_vit_accelerator_amd.ingest_wire_ref import ingest_wire_reference

pytestmark = pytest.mark.gpu

HEADER = "idx,timestamp,desired_vel,quat_1,quat_2,quat_3,quat_4,pos_x,pos_y,pos_z,vel_x,vel_y,vel_z,extra\n"
ORACLE_TOL = 2e-5


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
    blob = params.blob_from_record(fx, synth.float_params(0, E=64), E=64)
    eng = host.Engine(blob, device=0, reserve=64)
    eng.blob = blob
    yield eng
    eng.close()


def _codes(a):
    """what the reference host would feed the graph for this decoded PNG"""
    if a.dtype == np.uint16:
        a = (a >> 8).astype(np.uint8)
    return a if a.shape == (60, 90) else ingest_wire_reference(a[None])[0]


@pytest.mark.parametrize("schedule", ["steps", "sequence"])
def test_stb_resize_equals_walk_and_oracle_on_the_definitions_codes(tmp_path, engine, oracle, schedule):
    import torch
    root, arrays = _make_root(tmp_path, [[(np.uint8, 96, 128)] * 3, [(np.uint8, 96, 128)] * 2])
    res = replay.replay_frames(engine, str(root), schedule=schedule, resize="stb")
    assert engine.head_status() == 0
    assert [r.trajectory for r in res] == ["traj_00"] * 3 + ["traj_01"] * 2
    k0 = 0
    for traj in replay.scan_root(str(root)):
        hidden, oh, oc = None, None, None
        for k, a in enumerate(arrays[traj.name]):
            tel, codes = traj.telemetry[k], _codes(a)[None]
            dv = np.array([[tel.desired_velocity / 10.0]], np.float32)
            qt = np.array([tel.quaternion], np.float32)
            vel, hidden = engine.forward(torch.from_numpy(codes).cuda(), torch.from_numpy(dv).cuda(), torch.from_numpy(qt).cuda(), hidden)
            r = res[k0 + k]
            np.testing.assert_array_equal(r.output, vel.cpu().numpy()[0], err_msg=f"{r.trajectory}/{r.frame}")
            ov, oh, oc = oracle.forward(engine.blob, codes, dv, qt, oh, oc)
            err = float(np.abs(r.output - ov[0]).max())
            print(f"{r.trajectory}/{r.frame}: max |vel - oracle| = {err:.3e}")
            assert err <= ORACLE_TOL
        k0 += len(arrays[traj.name])


@pytest.mark.parametrize("schedule", ["steps", "sequence"])
def test_any_mix_of_sizes_and_depths_is_one_image_type(tmp_path, engine, schedule):
    """90 x 60 frames, two other sizes and a 16-bit PNG in one trajectory: every frame a u8 wire frame, state carried"""
    import torch
    mixed = [(np.uint8, 60, 90), (np.uint8, 96, 128), (np.uint16, 75, 100), (np.uint8, 45, 70)]
    root, arrays = _make_root(tmp_path, [mixed, [(np.uint8, 96, 128)] * 2], seed=1)
    res = replay.replay_frames(engine, str(root), schedule=schedule, resize="stb")
    assert engine.head_status() == 0 and len(res) == 6
    traj, hidden = replay.scan_root(str(root))[0], None
    for k, a in enumerate(arrays["traj_00"]):
        tel = traj.telemetry[k]
        vel, hidden = engine.forward(torch.from_numpy(_codes(a)[None]).cuda(),
                                     torch.tensor([tel.desired_velocity / 10.0], dtype=torch.float32, device="cuda"),
                                     torch.tensor([tel.quaternion], dtype=torch.float32, device="cuda"), hidden)
        np.testing.assert_array_equal(res[k].output, vel.cpu().numpy()[0])
