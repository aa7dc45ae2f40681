#!/usr/bin/env python3
"""Per-step time of a stream whose frames are all known up front, on the GPU box: Engine.forward_sequence against the step
schedules, in one process, u8 frames resident, for (T, B) = (1024, 1), (1024, 8), (512, 32), (128, 128), (16, 1024) on
an engine reserved for 1024 frames.  Candidates:
  a  forward      a loop of Engine.forward (state ping-pong, preallocated outputs)
  b  graphed      GraphedStep replays (one HIP-graph launch per step, static buffers)
  c  pipelined    PipelinedSteps(n_steps=8, stages=3) replays (eight steps per launch, three streams)
  d  sequence     Engine.forward_sequence, T steps per call (chunks of 1024 / B steps)
Every candidate of a shape is warmed first; then the candidates take turns -- a, b, c, d, a, b, c, d, ... for ROUNDS rounds,
each turn at least --min-seconds / ROUNDS of work bracketed by device synchronisations -- and a figure is the summed time
of a candidate's turns over their steps (at least --min-seconds of work per figure).  The whole table is taken twice so
that the spread is visible.  Prints one JSON (us per step and frames/s per cell and pass,
and the ratio d / best of a, b, c; "gate": that ratio is at most 0.6 at (1024, 1) and (1024, 8) in both
passes) and writes it to --out if given.
--only-sequence T,B: nothing but candidate d at one shape, --reps times, for a rocprofv3 --kernel-trace --stats run of its
own (time per ita_lstm_seq_kernel launch).
usage: python tools/bench_sequence.py [--out FILE] [--min-seconds S] [--only-sequence T,B --reps N]"""
import argparse, json, math, os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from drone_oa_iree_vit_accelerator_amd import host, params, synth

SHAPES = [(1024, 1), (1024, 8), (512, 32), (128, 128), (16, 1024)]
GATED = [(1024, 1), (1024, 8)]
GATE = 0.6
ROUNDS = 4

ap = argparse.ArgumentParser()
ap.add_argument("--out")
ap.add_argument("--min-seconds", type=float, default=0.5)
ap.add_argument("--only-sequence")
ap.add_argument("--reps", type=int, default=20)
a = ap.parse_args()

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
fx = params.load_fixture(os.path.join(REPO, "tests", "golden", "vitlstm_E64_seed0_B2.npz"))
eng = host.Engine(params.blob_from_record(fx, synth.float_params(0, E=64), E=64), device=0, reserve=1024)


def inputs(T, B):
    g = torch.Generator(device="cuda").manual_seed(T * 4099 + B)
    img = torch.randint(0, 256, (T, B, 60, 90), dtype=torch.uint8, device="cuda", generator=g)
    dv = torch.rand((T, B), device="cuda", generator=g) * 0.6 + 0.2
    qt = torch.randn((T, B, 4), device="cuda", generator=g)
    return img, dv, qt / qt.norm(dim=-1, keepdim=True)


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def turn(fn, reps):
    """reps calls of fn between two synchronisations -> seconds"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def candidates(T, B):
    img, dv, qt = inputs(T, B)
    state = [(torch.zeros((3, B, 128), device="cuda"), torch.zeros((3, B, 128), device="cuda")) for _ in range(2)]
    vel1 = torch.empty((B, 3), device="cuda")
    velT = torch.empty((T, B, 3), device="cuda")

    def forward():
        for t in range(T):
            eng.forward(img[t], dv[t], qt[t], state[t & 1], out=(vel1, *state[(t + 1) & 1]))

    gs = eng.graphed_step(B)
    gs.img.copy_(img[0]); gs.desvel.copy_(dv[0]); gs.quat.copy_(qt[0])

    def graphed():
        for _ in range(T):
            gs()

    ps = eng.pipelined_steps(B, n_steps=8, stages=3)
    ps.img.copy_(img[:8]); ps.desvel.copy_(dv[:8]); ps.quat.copy_(qt[:8])

    def pipelined():
        for _ in range(T // 8):
            ps()

    def sequence():
        eng.forward_sequence(img, dv, qt, state[0], out=(velT, *state[0]))

    return [("forward", forward), ("graphed", graphed), ("pipelined", pipelined), ("sequence", sequence)], (gs, ps)


if a.only_sequence:
    T, B = (int(x) for x in a.only_sequence.split(","))
    img, dv, qt = inputs(T, B)
    h, c = torch.zeros((3, B, 128), device="cuda"), torch.zeros((3, B, 128), device="cuda")
    vel = torch.empty((T, B, 3), device="cuda")
    for _ in range(a.reps):
        eng.forward_sequence(img, dv, qt, (h, c), out=(vel, h, c))
    torch.cuda.synchronize()
    assert eng.head_status() == 0
    print(json.dumps({"only_sequence": [T, B], "reps": a.reps}))
    sys.exit(0)

passes = []
for p in range(2):
    table = {}
    for T, B in SHAPES:
        cands, keep = candidates(T, B)
        for _, fn in cands:      # warm every candidate of the shape before the first figure
            fn()
        torch.cuda.synchronize()
        reps = {name: max(1, int(math.ceil(a.min_seconds / ROUNDS / max(once(fn), 1e-6)))) for name, fn in cands}
        secs = {name: 0.0 for name, _ in cands}
        for _ in range(ROUNDS):
            for name, fn in cands:
                secs[name] += turn(fn, reps[name])
        cell = {}
        for name, _ in cands:
            us = secs[name] / (ROUNDS * reps[name] * T) * 1e6
            cell[name] = {"us_per_step": round(us, 3), "frames_per_s": round(B / us * 1e6)}
        best = min(cell[k]["us_per_step"] for k in ("forward", "graphed", "pipelined"))
        cell["sequence_over_best_step_schedule"] = round(cell["sequence"]["us_per_step"] / best, 4)
        table[f"{T}x{B}"] = cell
        del cands, keep
        print(f"pass {p} T={T} B={B}: {json.dumps(cell)}", file=sys.stderr, flush=True)
    passes.append(table)
assert eng.head_status() == 0
gate = {f"{T}x{B}": [ps[f"{T}x{B}"]["sequence_over_best_step_schedule"] for ps in passes] for T, B in GATED}
res = {"tool": "tools/bench_sequence.py", "device": torch.cuda.get_device_name(0), "reserved_frames": 1024,
       "min_seconds_per_figure": a.min_seconds, "rounds_per_figure": ROUNDS, "passes": passes,
       "gate": {"bound": GATE, "ratios": gate, "met": all(r <= GATE for v in gate.values() for r in v)}}
out = json.dumps(res, indent=1)
print(out)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(out + "\n")
