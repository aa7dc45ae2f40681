#!/usr/bin/env python3
"""Time of the ingest stage (Engine.ingest: camera-resolution frames -> (N,60,90) f32) on the GPU box, beside the route the
engine had before it, in one process:
  ingest   Engine.ingest(raw, out=...)                      one HIP kernel, reads only the source rows the blend needs
  torch    raw.float().div(255) then F.interpolate(..., size=(60, 90), mode="bilinear", align_corners=False)
           (f32 sources: the interpolate alone; u16 sources: raw.float().mul(1 / 65535).clamp(max=1) in front of it where
           this torch build converts uint16 on the GPU, else "no route" -- the engine never had one for 16-bit frames)
Shapes: 480 x 640 u8 and u16 at 1, 128 and 1024 frames per call, 120 x 180 f32 at 1024.
Source buffers rotate through a pool whose rows touched by ingest alone come to at least --pool-mb (default 640 MB,
beyond the 256 MiB Infinity Cache; the pool itself is 2.6 GB for the 480-row shapes) so that no call finds its rows in
a cache; both candidates of a shape are warmed, then take turns for ROUNDS rounds, each turn at least --min-seconds /
ROUNDS of calls between two device synchronisations.  These are times per CALL: at 1 and 128 frames they are the rate at
which the host enqueues, not the kernel (--only below).  Reported per shape and candidate: us per
call of every round (min / median / max), and for ingest the achieved GB/s over the bytes-touched model (the distinct
source rows the 60 output rows blend + the f32 output) and its fraction of a 6.0 TB/s streaming rate -- except where the
call takes less than 1.5 x a one-frame call: such a time is the host's, and no bandwidth is derived from it
("host_call_rate_bound").
Prints one JSON and writes it to --out if given.
--only DT,N: nothing but Engine.ingest at one shape (u8 / u16 at 480 x 640, f32 at 120 x 180), --reps calls over the
rotating pool, for a rocprofv3 --kernel-trace --stats run of its own (time per kernel launch).
usage: python tools/bench_ingest.py [--out FILE] [--min-seconds S] [--pool-mb MB] [--only DT,N --reps R]"""
import argparse, json, math, os, statistics, sys, time
import numpy as np
import torch
import torch.nn.functional as F
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from drone_oa_iree_vit_accelerator_amd import host, ingest_ref, params, synth

SHAPES = [("u8", 480, 640, 1), ("u8", 480, 640, 128), ("u8", 480, 640, 1024),
          ("u16", 480, 640, 1), ("u16", 480, 640, 128), ("u16", 480, 640, 1024),
          ("f32", 120, 180, 1024)]
ROUNDS = 5
STREAM_TBS = 6.0

ap = argparse.ArgumentParser()
ap.add_argument("--out")
ap.add_argument("--min-seconds", type=float, default=0.5)
ap.add_argument("--pool-mb", type=float, default=640.0)
ap.add_argument("--only")
ap.add_argument("--reps", type=int, default=2000)
a = ap.parse_args()

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
fx = params.load_fixture(os.path.join(REPO, "tests", "golden", "vitlstm_E64_seed0_B2.npz"))
eng = host.Engine(params.blob_from_record(fx, synth.float_params(0, E=64), E=64), device=0)
PIX = {"u8": 1, "u16": 2, "f32": 4}


def bytes_touched(dt, H, W, N):
    y0, y1, _, _ = ingest_ref.axis_table(H, 60)
    rows = len(set(y0.tolist()) | set(y1.tolist()))
    return N * rows * W * PIX[dt], N * 60 * 90 * 4


def pool(dt, H, W, N):
    """windows of N frames over a pool of random frames large enough that the source rows ingest TOUCHES in one sweep of
    the pool (a quarter of a 480-row frame) come to at least --pool-mb"""
    n_win = max(2, int(math.ceil(a.pool_mb * 1e6 / bytes_touched(dt, H, W, N)[0])))
    g = torch.Generator(device="cuda").manual_seed(H * 4099 + W + N)
    if dt == "f32":
        p = torch.rand((n_win * N, H, W), device="cuda", generator=g)
    elif dt == "u8":
        p = torch.randint(0, 256, (n_win * N, H, W), dtype=torch.uint8, device="cuda", generator=g)
    else:
        p = torch.randint(0, 256, (n_win * N, H, 2 * W), dtype=torch.uint8, device="cuda", generator=g).view(torch.uint16)
    return [p[i * N:(i + 1) * N] for i in range(n_win)]


def torch_route(dt):
    def resize(x):
        return F.interpolate(x[:, None], size=(60, 90), mode="bilinear", align_corners=False)
    if dt == "u8":
        return lambda raw: resize(raw.float().div(255))
    if dt == "u16":
        return lambda raw: resize(raw.float().mul(1.0 / 65535.0).clamp(max=1.0))
    return resize


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


if a.only:
    dt, N = a.only.split(",")
    N = int(N)
    H, W = (120, 180) if dt == "f32" else (480, 640)
    wins = pool(dt, H, W, N)
    out = torch.empty((N, 60, 90), device="cuda")
    turn(lambda raw: eng.ingest(raw, out=out), wins, 0, a.reps)
    print(json.dumps({"only": [dt, H, W, N], "reps": a.reps, "source_windows": len(wins)}))
    eng.close()
    sys.exit(0)

table, one_frame = {}, {}
for dt, H, W, N in SHAPES:
    wins = pool(dt, H, W, N)
    out = torch.empty((N, 60, 90), device="cuda")
    cands = [("ingest", lambda raw: eng.ingest(raw, out=out))]
    route = torch_route(dt)
    try:
        got = route(wins[0])[:, 0]
        torch.cuda.synchronize()
        cands.append(("torch", route))
        dev = float((got - eng.ingest(wins[0])).abs().max())      # same frames, both routes: they agree to rounding
    except (RuntimeError, TypeError) as e:
        dev, route_error = None, str(e).splitlines()[0][:120]
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
    src_b, out_b = bytes_touched(dt, H, W, N)
    med = statistics.median(us["ingest"])
    # a call that takes no longer than 1.5 x a one-frame call (the shortest measured so far; the list starts with one) is
    # timed by the host's enqueue rate, not by the kernel: bytes over such a time are not a bandwidth, so none is reported
    if N == 1:
        one_frame[dt] = med
    host_bound = med < 1.5 * min(one_frame.values())
    cell = {"source_windows": len(wins), "pool_mb": round(len(wins) * N * H * W * PIX[dt] / 1e6, 1),
            "pool_mb_touched_by_ingest": round(len(wins) * src_b / 1e6, 1),
            "bytes_model": {"source_rows": src_b, "output": out_b},
            "ingest_us": box(us["ingest"]), "ingest_calls_per_round": reps["ingest"],
            "host_call_rate_bound": host_bound,
            "ingest_gb_per_s": None if host_bound else round((src_b + out_b) / med / 1e3, 1),
            "ingest_fraction_of_6TBs": None if host_bound else round((src_b + out_b) / med / 1e3 / (STREAM_TBS * 1e3), 4)}
    if "torch" in us:
        cell.update({"torch_us": box(us["torch"]), "torch_calls_per_round": reps["torch"],
                     "torch_over_ingest": round(statistics.median(us["torch"]) / med, 2),
                     "max_abs_difference_of_the_two_routes": dev})
    else:
        cell.update({"torch_us": None, "torch_route_error": route_error})
    table[f"{dt}_{H}x{W}_n{N}"] = cell
    print(f"{dt} {H}x{W} n={N}: {json.dumps(cell)}", file=sys.stderr, flush=True)
    del wins, out, cands
    torch.cuda.empty_cache()

res = {"tool": "tools/bench_ingest.py", "device": torch.cuda.get_device_name(0), "min_seconds_per_figure": a.min_seconds,
       "rounds_per_figure": ROUNDS, "streaming_rate_TBs": STREAM_TBS, "shapes": table}
text = json.dumps(res, indent=1)
print(text)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
eng.close()
