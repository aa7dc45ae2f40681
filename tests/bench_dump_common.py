"""What bench.py --dump-outputs must have written: the same number of sequential ita_vitlstm_forward calls from zero state
on the bench's own seeded inputs.  Shared by test_gpu_bench_dump.py and test_gpu_bench_multi.py; needs a GPU."""
import os

import numpy as np

from conftest import REPO


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
