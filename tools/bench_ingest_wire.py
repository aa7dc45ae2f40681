#!/usr/bin/env python3
"""Time of the wire ingest (Engine.ingest_wire: camera-resolution u8 frames -> (N,60,90) u8 wire frames, the reference
host's stb resize) on the GPU box, in one process:
  wire     Engine.ingest_wire(raw, out=...)                  one HIP kernel, reads every source byte
  torch    F.interpolate(raw.float()[:, None], (60, 90), mode="bilinear", antialias=True), then round, clamp and cast
           to uint8 -- the nearest torch route.  ANOTHER filter (a triangle, not Mitchell): a timing comparator only.
  floor    the bytes of the call (source + output) at the 6.0 TB/s streaming rate
Shapes: 480 x 640 u8 at 1, 128 and 1024 frames per call.  Then the step at 1024 frames, end to end:
  wire_step    Engine.forward(Engine.ingest_wire(raw, out=...), desvel)     u8 wire frames: tokenizer fused into the encoder
  f32_step     Engine.forward(Engine.ingest(raw, out=...), desvel)          f32 frames: stand-alone tokenizer
Source buffers rotate through a pool of at least --pool-mb (default 640 MB, beyond the 256 MiB Infinity Cache); the
candidates of a shape are warmed, then take turns for ROUNDS rounds, each turn at least --min-seconds / ROUNDS of calls
between two device synchronisations.  These are times per CALL: at 1 frame they are the rate at which the host enqueues.
Prints one JSON and writes it to --out if given.
usage: python tools/bench_ingest_wire.py [--out FILE] [--min-seconds S] [--pool-mb MB]"""
import argparse, json, math, os, statistics, sys, time
import torch
import torch.nn.functional as F
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from drone_oa_iree_vit_accelerator_amd import host, params, synth

H, W = 480, 640
BATCHES = [1, 128, 1024]
ROUNDS = 5
STREAM_TBS = 6.0

ap = argparse.ArgumentParser()
ap.add_argument("--out")
ap.add_argument("--min-seconds", type=float, default=0.5)
ap.add_argument("--pool-mb", type=float, default=640.0)
a = ap.parse_args()

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
fx = params.load_fixture(os.path.join(REPO, "tests", "golden", "vitlstm_E64_seed0_B2.npz"))
eng = host.Engine(params.blob_from_record(fx, synth.float_params(0, E=64), E=64), device=0, reserve=max(BATCHES))
eng.prepare_ingest_wire(H, W)


def pool(N):
    n_win = max(2, int(math.ceil(a.pool_mb * 1e6 / (N * H * W))))
    g = torch.Generator(device="cuda").manual_seed(N)
    p = torch.randint(0, 256, (n_win * N, H, W), dtype=torch.uint8, device="cuda", generator=g)
    return [p[i * N:(i + 1) * N] for i in range(n_win)]


def torch_route(raw):
    y = F.interpolate(raw.float()[:, None], size=(60, 90), mode="bilinear", antialias=True)
    return y.round().clamp(0, 255).to(torch.uint8)


def turn(fn, wins, start, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(reps):
        fn(wins[(start + i) % len(wins)])
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def box(us):
    return {"min": round(min(us), 3), "median": round(statistics.median(us), 3), "max": round(max(us), 3),
            "rounds": [round(u, 3) for u in us]}


def alternate(cands, wins):
    reps, start = {}, {}
    for name, fn in cands:                                         # warm, then size a turn
        turn(fn, wins, 0, 3)
        reps[name] = max(3, int(math.ceil(a.min_seconds / ROUNDS / max(turn(fn, wins, 0, 3) / 3, 1e-6))))
        start[name] = 0
    us = {name: [] for name, _ in cands}
    for _ in range(ROUNDS):
        for name, fn in cands:
            us[name].append(turn(fn, wins, start[name], reps[name]) / reps[name] * 1e6)
            start[name] = (start[name] + reps[name]) % len(wins)
    return us, reps


table = {}
for N in BATCHES:
    wins = pool(N)
    out = torch.empty((N, 60, 90), dtype=torch.uint8, device="cuda")
    us, reps = alternate([("wire", lambda raw: eng.ingest_wire(raw, out=out)), ("torch", torch_route)], wins)
    nbytes = N * (H * W + 60 * 90)
    med = statistics.median(us["wire"])
    cell = {"source_windows": len(wins), "pool_mb": round(len(wins) * N * H * W / 1e6, 1), "bytes": nbytes,
            "floor_us_at_6TBs": round(nbytes / (STREAM_TBS * 1e6), 3),
            "wire_us": box(us["wire"]), "wire_calls_per_round": reps["wire"],
            "wire_gb_per_s": round(nbytes / med / 1e3, 1), "wire_fraction_of_6TBs": round(nbytes / med / 1e3 / (STREAM_TBS * 1e3), 4),
            "torch_us": box(us["torch"]), "torch_calls_per_round": reps["torch"],
            "torch_over_wire": round(statistics.median(us["torch"]) / med, 2),
            "largest_code_difference_of_the_two_filters": int((torch_route(wins[0]).int() - eng.ingest_wire(wins[0]).int()).abs().max())}
    if N == max(BATCHES):
        dv = torch.full((N,), 0.5, device="cuda")
        f32 = torch.empty((N, 60, 90), device="cuda")
        us2, reps2 = alternate([("wire_step", lambda raw: eng.forward(eng.ingest_wire(raw, out=out), dv)),
                                ("f32_step", lambda raw: eng.forward(eng.ingest(raw, out=f32), dv))], wins)
        cell["step"] = {"wire_step_us": box(us2["wire_step"]), "f32_step_us": box(us2["f32_step"]),
                        "calls_per_round": reps2,
                        "f32_over_wire": round(statistics.median(us2["f32_step"]) / statistics.median(us2["wire_step"]), 3)}
    table[f"u8_{H}x{W}_n{N}"] = cell
    print(f"n={N}: {json.dumps(cell)}", file=sys.stderr, flush=True)
    del wins, out
    torch.cuda.empty_cache()

res = {"tool": "tools/bench_ingest_wire.py", "device": torch.cuda.get_device_name(0), "min_seconds_per_figure": a.min_seconds,
       "rounds_per_figure": ROUNDS, "streaming_rate_TBs": STREAM_TBS, "shapes": table}
text = json.dumps(res, indent=1)
print(text)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
eng.close()
