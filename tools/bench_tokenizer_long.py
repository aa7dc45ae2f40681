#!/usr/bin/env python3
"""Time of the long-sequence tokenizer (Engine.tokenize_long) on the GPU box at BASELINE config 5 -- 32 frames of 480 x 720
-> 64 x 128 = 8192 tokens per frame -- at E = 128 and E = 64, on u8 and f32 frames, beside what a user had to write
before it existed, in one process:

  entry   Engine.tokenize_long(frames, 64, 128, out=...): one HIP kernel, the 7 x 7 patches blended first
  torch   F.conv2d(stride 2, padding 3) -> F.interpolate(size=(64, 128), bilinear, align_corners=False) -> flatten,
          transpose -> F.layer_norm, on the same GPU with the same parameters (u8 frames: .float().div(255) in front);
          it writes and re-reads the (32, E, 240, 360) f32 conv map
  floor   the frame bytes once plus the token bytes once at the 6.0 TB/s streaming rate tools/bench_ingest.py uses

Source frames rotate through a pool of at least --pool-mb (default 640 MB, beyond the 256 MiB Infinity Cache), so no call
finds its frames in a cache.  Both candidates of a shape are warmed, then take turns for ROUNDS rounds, each turn at least
--min-seconds / ROUNDS of calls between two device synchronisations; min / median / max of the rounds, us per call.  The
two routes' outputs are compared once per shape (they agree to float rounding).

One more row times the entry's other form (E = 128, u8, 64 x 32 tokens: a horizontal ratio of 11.25, where the kernel
loads its pixels directly instead of through its LDS window).  Then the whole chain at E = 128, two int8 layers, 48 output
channels, as tools/bench_long_layer.py times it from resident tokens:
  frames_chain  encode_frames_long(u8 frames) -> ita_fusion_tail_large
  tokens_chain  encode_long(tokens) -> same

--only E,DT: nothing but the entry at one shape, --reps calls over the rotating pool, for a rocprofv3 --kernel-trace --stats
run of its own (time per kernel launch).
usage: python tools/bench_tokenizer_long.py [--out FILE] [--min-seconds S] [--pool-mb MB] [--frames N] [--only E,DT --reps R]"""
import argparse, json, math, os, statistics, sys, time
import torch
import torch.nn.functional as F
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from drone_oa_iree_vit_accelerator_amd import host, params, synth

H, W, TH, TW = 480, 720, 64, 128
ROUNDS = 5
STREAM_TBS = 6.0
PIX = {"u8": 1, "f32": 4}
GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")

ap = argparse.ArgumentParser()
ap.add_argument("--out")
ap.add_argument("--min-seconds", type=float, default=0.5)
ap.add_argument("--pool-mb", type=float, default=640.0)
ap.add_argument("--frames", type=int, default=32)
ap.add_argument("--only")
ap.add_argument("--reps", type=int, default=200)
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_tokenizer_long.py measures on the GPU: none visible")
N = a.frames


def engine(E):
    if E == 64:
        d, nl, fp = params.load_fixture(os.path.join(GOLDEN, "vitlstm_E64_seed0_B2.npz")), 1, synth.float_params(0, E=64)
    else:
        d, nl = params.load_fixture(os.path.join(GOLDEN, "vit2l_E128_s0_B2.npz")), 2
        fp = synth.float_params(0, E=128, num_layers=2, tail=False)
    return host.Engine(params.blob_from_record(d, fp, E=E, num_layers=nl), device=0), fp


def pool(dt):
    n_win = max(2, int(math.ceil(a.pool_mb * 1e6 / (N * H * W * PIX[dt]))))
    g = torch.Generator(device="cuda").manual_seed(4099 + PIX[dt])
    if dt == "f32":
        p = torch.rand((n_win * N, H, W), device="cuda", generator=g)
    else:
        p = torch.randint(0, 256, (n_win * N, H, W), dtype=torch.uint8, device="cuda", generator=g)
    return [p[i * N:(i + 1) * N] for i in range(n_win)]


def torch_route(fp, dt):
    cw, cb = torch.from_numpy(fp["tokenizer.conv.weight"]).cuda(), torch.from_numpy(fp["tokenizer.conv.bias"]).cuda()
    lw, lb = torch.from_numpy(fp["tokenizer.norm.weight"]).cuda(), torch.from_numpy(fp["tokenizer.norm.bias"]).cuda()
    E = cw.shape[0]

    def route(raw):
        x = raw.float().div(255) if dt == "u8" else raw
        x = F.conv2d(x[:, None], cw, cb, stride=2, padding=3)
        x = F.interpolate(x, size=(TH, TW), mode="bilinear", align_corners=False)
        return F.layer_norm(x.flatten(2).transpose(1, 2), (E,), lw, lb)
    return route


def turn(fn, wins, start, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(reps):
        fn(wins[(start + i) % len(wins)])
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def box(us):
    return {"min": round(min(us), 2), "median": round(statistics.median(us), 2), "max": round(max(us), 2),
            "rounds": [round(u, 2) for u in us]}


def race(cands, wins):
    """cands: [(name, fn(window))] -> {name: us per call of every round}, the candidates taking turns"""
    reps, start = {}, {}
    for name, fn in cands:
        turn(fn, wins, 0, 3)
        reps[name] = max(3, int(math.ceil(a.min_seconds / ROUNDS / max(turn(fn, wins, 0, 3) / 3, 1e-6))))
        start[name] = 0
    us = {name: [] for name, _ in cands}
    for _ in range(ROUNDS):
        for name, fn in cands:
            us[name].append(turn(fn, wins, start[name], reps[name]) / reps[name] * 1e6)
            start[name] = (start[name] + reps[name]) % len(wins)
    return us, reps


if a.only:
    E, dt = a.only.split(",")
    eng, _ = engine(int(E))
    wins = pool(dt)
    out = torch.empty((N, TH * TW, eng.E), device="cuda")
    turn(lambda raw: eng.tokenize_long(raw, TH, TW, out=out), wins, 0, a.reps)
    print(json.dumps({"only": [int(E), dt, H, W, N], "reps": a.reps, "source_windows": len(wins)}))
    eng.close()
    sys.exit(0)

table = {}
for E in (128, 64):
    eng, fp = engine(E)
    for dt in ("u8", "f32"):
        wins = pool(dt)
        out = torch.empty((N, TH * TW, E), device="cuda")
        route = torch_route(fp, dt)
        dev = float((route(wins[0]) - eng.tokenize_long(wins[0], TH, TW)).abs().max())
        us, reps = race([("entry", lambda raw: eng.tokenize_long(raw, TH, TW, out=out)), ("torch", route)], wins)
        frame_b, token_b = N * H * W * PIX[dt], N * TH * TW * E * 4
        floor_us = (frame_b + token_b) / (STREAM_TBS * 1e12) * 1e6
        med = statistics.median(us["entry"])
        cell = {"source_windows": len(wins), "pool_mb": round(len(wins) * frame_b / 1e6, 1),
                "bytes_model": {"frames": frame_b, "tokens": token_b}, "byte_floor_us": round(floor_us, 2),
                "entry_us": box(us["entry"]), "entry_calls_per_round": reps["entry"],
                "entry_over_byte_floor": round(med / floor_us, 2),
                "entry_gmac_per_s": round(N * TH * TW * E * 49 / med / 1e3, 1),
                "torch_us": box(us["torch"]), "torch_calls_per_round": reps["torch"],
                "torch_over_entry": round(statistics.median(us["torch"]) / med, 2),
                "max_abs_difference_of_the_two_routes": dev}
        table[f"E{E}_{dt}_{H}x{W}_n{N}"] = cell
        print(f"E{E} {dt}: {json.dumps(cell)}", file=sys.stderr, flush=True)
        del wins, out, route
        torch.cuda.empty_cache()
    if E == 128:      # the other form of the kernel: 64 x 32 tokens, horizontal ratio 11.25, no LDS window (direct loads)
        wins = pool("u8")
        out = torch.empty((N, TH * 32, E), device="cuda")
        us, reps = race([("entry", lambda raw: eng.tokenize_long(raw, TH, 32, out=out))], wins)
        frame_b, token_b = N * H * W, N * TH * 32 * E * 4
        floor_us = (frame_b + token_b) / (STREAM_TBS * 1e12) * 1e6
        table[f"E{E}_u8_{H}x{W}_n{N}_T{TH}x32_direct_loads"] = {
            "bytes_model": {"frames": frame_b, "tokens": token_b}, "byte_floor_us": round(floor_us, 2), "entry_us": box(us["entry"]),
            "entry_calls_per_round": reps["entry"], "entry_over_byte_floor": round(statistics.median(us["entry"]) / floor_us, 2)}
        del wins, out
        torch.cuda.empty_cache()
    if E == 128:      # the whole chain: frames (or resident tokens) -> two encoder layers -> large-grid fusion tail
        c = synth.tail_large_case(0, E, TH, TW, 48, 1)
        tail = host.FusionTailLarge(c["conv_w"], c["conv_b"], device=0)
        fmap = torch.empty((N, 48, 2 * TH, 2 * TW), device="cuda")
        wins = pool("u8")
        tok = eng.tokenize_long(wins[0], TH, TW)
        us, reps = race([("frames_chain", lambda raw: tail(eng.encode_frames_long(raw, TH, TW), TH, TW, out=fmap)),
                         ("tokens_chain", lambda raw: tail(eng.encode_long(tok), TH, TW, out=fmap))], wins)
        table["chain_E128_u8"] = {"layers": eng.num_layers, "tail_outputs": 48,
                                  "frames_chain_us": box(us["frames_chain"]), "tokens_chain_us": box(us["tokens_chain"]),
                                  "calls_per_round": reps,
                                  "frames_over_tokens": round(statistics.median(us["frames_chain"]) / statistics.median(us["tokens_chain"]), 4)}
        print(f"chain: {json.dumps(table['chain_E128_u8'])}", file=sys.stderr, flush=True)
        tail.close()
        del wins, tok, fmap
        torch.cuda.empty_cache()
    eng.close()

res = {"tool": "tools/bench_tokenizer_long.py", "device": torch.cuda.get_device_name(0), "frames_per_call": N,
       "frame": [H, W], "token_grid": [TH, TW], "min_seconds_per_figure": a.min_seconds, "rounds_per_figure": ROUNDS,
       "streaming_rate_TBs": STREAM_TBS, "unit": "us per call", "shapes": table}
text = json.dumps(res, indent=1)
print(text)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
