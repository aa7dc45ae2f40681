"""bench.py --dump-outputs on one GPU: a plain run prints the headline line only, and what it writes is what its last
timed step returned -- equal, bit for bit, to the same number of sequential ita_vitlstm_forward calls from zero state on
the bench's own seeded inputs (warm-up and timed steps carry the state as one sequence when --warmup is even and there
are no settle steps)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu


def sequential_forward(sizes, n_steps):
    """velocities of every rank's frames (bench.py: synth.frames(1234 + rank, shard)) after n_steps forwards, and rank 0's
    (h, c)"""
    import torch
    from drone_oa_iree_vit_accelerator_amd import host, params, synth
    fx = params.load_fixture(os.path.join(REPO, "tests", "golden", "vitlstm_E64_seed0_B2.npz"))
    eng = host.Engine(params.blob_from_record(fx, synth.float_params(0, E=64), E=64), device=0)
    vels, state0 = [], None
    for rank, B in enumerate(sizes):
        fr = synth.frames(1234 + rank, B)
        img, dv, qt = (torch.from_numpy(fr[k]).cuda() for k in ("img_u8", "desvel", "quat"))
        st = None
        for _ in range(n_steps):
            v, st = eng.forward(img, dv, qt, st)
        vels.append(v.cpu().numpy())
        if rank == 0:
            state0 = tuple(s.cpu().numpy() for s in st)
    eng.close()
    return np.concatenate(vels), state0


def check_dump(path, sizes, n_steps):
    vel, (h, c) = sequential_forward(sizes, n_steps)
    got = {n: np.load(os.path.join(path, n + ".npy")) for n in ("velocity", "h", "c")}
    assert sorted(os.listdir(path)) == ["c.npy", "h.npy", "velocity.npy"]
    assert all(x.dtype == np.float32 for x in got.values())
    np.testing.assert_array_equal(got["velocity"], vel)
    np.testing.assert_array_equal(got["h"], h)
    np.testing.assert_array_equal(got["c"], c)


@pytest.mark.parametrize("schedule", ["stream", "graph"])
def test_plain_run_dumps_last_step(tmp_path, schedule):
    B, K, W = 64, 16, 8
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(K), "--warmup", str(W),
           "--frames-per-gpu", str(B), "--settle-steps", "0", "--schedule", schedule, "--dump-outputs", str(tmp_path)]
    r = subprocess.run(cmd, cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    lines = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout.decode()[-2000:]
    out = json.loads(lines[0])
    assert out["steps"] == K and out["unit"] == "frames/s" and out["higher_is_better"] is True and out["dtype"] == "int8+f32"
    assert abs(out["value"] - B / (out["ms_per_step"] * 1e-3)) <= 1e-3 * out["value"]
    assert not {"roofline", "stages", "cpu_baseline", "configs", "p50_latency_ms_b1"} & set(out)     # --full only
    check_dump(str(tmp_path), [B], W + K)
