"""replay(schedule="sequence") -- whole trajectories through Engine.forward_sequence -- returns what the default step
schedule returns: the same frames in the same order, outputs bit-equal, errors equal.  The synthetic root is built as
tests/test_replay.py builds its own (three trajectories of 4, 2 and 5 frames, one corrupt PNG in the middle of one)."""
import os

import numpy as np
import pytest

from drone_oa_iree_vit_accelerator_amd import host, params, replay, synth

pytestmark = pytest.mark.gpu

HEADER = "idx,timestamp,desired_vel,quat_1,quat_2,quat_3,quat_4,pos_x,pos_y,pos_z,vel_x,vel_y,vel_z,extra\n"


def _make_root(tmp_path, lens=(4, 2, 5), seed=0):
    from PIL import Image
    rs = np.random.RandomState(seed)
    root = tmp_path / "data"
    root.mkdir()
    for t, n in enumerate(lens):
        d = root / f"traj_{t:02d}"
        d.mkdir()
        rows = [HEADER]
        for k in range(n):
            ts = 100.0 + t + 0.1 * k
            Image.fromarray(rs.randint(0, 256, size=(60, 90)).astype(np.uint8)).save(str(d / f"{ts:.3f}.png"))
            dv = float(rs.uniform(2, 8))
            q = rs.standard_normal(4)
            q /= np.linalg.norm(q)
            gt = rs.standard_normal(3)
            rows.append(f"{k},{ts + 0.0004:.4f},{dv:.6f},{q[0]:.6f},{q[1]:.6f},{q[2]:.6f},{q[3]:.6f},0,0,0,"
                        f"{gt[0]:.6f},{gt[1]:.6f},{gt[2]:.6f},x\n")
        (d / "data.csv").write_text("".join(rows))
    return root


@pytest.mark.parametrize("max_batch", [1024, 2])
def test_sequence_schedule_equals_step_schedule(tmp_path, max_batch):
    root = _make_root(tmp_path, seed=3)
    (root / "traj_01" / "101.050.png").write_bytes(b"corrupt")   # sorts between traj_01's two frames: dropped from the sequence
    (root / "traj_02" / "102.250.png").write_bytes(b"corrupt")   # in the middle of the longest trajectory
    fx = params.load_fixture(os.path.join(os.path.dirname(__file__), "golden", "vitlstm_E64_seed0_B2.npz"))
    # 64 frames of workspace: every group (3 trajectories x 5 steps; with max_batch 2: 2 x 4, then 1 x 4) is one launch
    eng = host.Engine(params.blob_from_record(fx, synth.float_params(0, E=64), E=64), device=0, reserve=64)
    ref = replay.replay(eng, str(root))
    assert [r.trajectory for r in ref] == ["traj_00"] * 4 + ["traj_01"] * 2 + ["traj_02"] * 5
    got = replay.replay(eng, str(root), max_batch=max_batch, schedule="sequence")
    assert eng.head_status() == 0
    assert [(r.trajectory, r.frame) for r in got] == [(r.trajectory, r.frame) for r in ref]
    for g, r in zip(got, ref):
        np.testing.assert_array_equal(g.output, r.output, err_msg=f"{r.trajectory}/{r.frame}")
        np.testing.assert_array_equal(g.ground_truth, r.ground_truth)
        assert g.error == r.error and g.telemetry_found == r.telemetry_found
    eng.close()
