"""bench.py --dump-outputs on one GPU: a plain run prints the headline line only, and what it writes is what its last
timed step returned -- equal, bit for bit, to the same number of sequential ita_vitlstm_forward calls from zero state on
the bench's own seeded inputs (warm-up and timed steps carry the state as one sequence when --warmup is even and there
are no settle steps)."""
import json
import os
import subprocess
import sys

import pytest

from bench_dump_common import check_dump
from conftest import REPO

pytestmark = pytest.mark.gpu


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
