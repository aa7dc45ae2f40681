#!/usr/bin/env python3
"""bench.py -- frames/s of the ITAViTLSTM int8 forward on MI355X (BASELINE.json metric).

  python bench.py --gpus N --steps K --warmup W [--full] [--dump-outputs DIR]
  (N > 1: python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 ... bench.py --gpus N ...)

One "step" = one pass of module.main_graph (tokenizer -> int8 MHA -> int8 FFN -> fusion tail ->
decoder -> 3-layer LSTM -> fc) over one batch of synthetic 60x90 depth frames per GPU
(BASELINE config 4: 1024 frames), inputs resident in HBM in the reference's wire format (u8 pixels,
--image-dtype f32 for the graph's own f32 input), LSTM state carried from step to step,
plus -- for N > 1 -- the RCCL all-gather of the (frames, 3) velocities.  Weak scaling: every GPU
always processes `--frames-per-gpu` independent streams.

Prints ONE JSON line (rank 0): frames/s over exactly K timed steps and ms_per_step.  A plain run does nothing else.
--dump-outputs DIR writes what the last timed step returned to its caller as float32 .npy files: velocity (all GPUs'
frames, gathered), h and c (3, frames, 128) of rank 0 (over 64 MB in all: the same seeded sample of frames in each).
--full adds these objects (--no-cpu-baseline / --no-latency / --no-configs drop single legs of it):
  roofline      dominant kernel: algorithmic ops per launch / its HIP-event time measured in the
                timed region, against the MI355X peak for its arithmetic (guide: int8 MFMA
                5.0 POP/s dense, f32 157.3 TFLOP/s)
  cpu_baseline  on the box's host cores, a bounded sample of the same workload (N = 1 only): the float twin of the graph in
                PyTorch f32 eager (kind "torch-f32-eager": what the reference's llvm-cpu .vmfb holds) and, under "port", the
                scalar int8 oracle (oracle/ita_oracle.c), one process per core and one core alone
  configs       c2: BASELINE config 2 (int8 MHA block alone: B = 1 latency, 1024-frame int8 MFMA fraction);
                c5: BASELINE config 5 (fusion tail on a 64x128 token grid: MFMA and HBM fractions), same run (N = 1 only);
                c5_mha: config 5 as worded, the int8 attention block on 8192 tokens per frame (three-sweep integer softmax);
                vit2l: the second graph family (E = 128, two layers, no fusion tail), whole forward at 1024 frames;
                b1 / b128 / b256: step time of the whole forward at 1, 128, 256 frames per GPU (config 3; config 4 cut over 8 GPUs)
  stages        per-stage times from an untimed eager pass with events around every stage
  p50_latency_ms_b1[_hipgraph]  single-frame latency, host enqueue -> result
--schedule selects one stream / the library's two-stream pipeline / its HIP-graph form (default: graph up to 256 frames per GPU).
--global-batch G gives the strong-scaling form of config 4 (G frames per step cut over the GPUs, "scaling": "strong").
"""
import argparse
import glob
import contextlib
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402

# algorithmic work per frame (BASELINE.md section 2 / SURVEY.md section 8(d)); E=64, S=128, P=192, F=256
STAGE_WORK = {   # stage: (ops per frame, bound, peak in Tera-op/s, arithmetic)
    "tokenizer": (2 * 4.23e6, "mfma", 157.3, "f32"),
    # int8 MHA + int8 FFN (+ both LayerNorms) are ONE launch: ita_stream_kernel
    "encoder": (2 * (12.58e6 + 4.19e6), "mfma", 5000.0, "int8"),
    # fusion conv + decoder run as ONE folded GEMM on split-precision f16 MFMA (priced against the
    # dense f16 peak with the reference graph's algorithmic flops, not the 3x split products)
    "tail_decoder": (2 * (3.32e6 + 2.36e6), "mfma", 2500.0, "f16x3"),
    "lstm_fc": (2 * 0.59e6, "mfma", 2500.0, "f16x3"),
}


# dominant-stage -> kernel whose PMC traffic (profiles/kernel_traffic.json, collected with
# tools/profile_gpu.sh on this same command) is reported as roofline.traffic
STAGE_KERNEL = {"encoder": "ita_stream_kernel<64, true, 1, false, false, true>", "tokenizer": "ita_tok_stream_kernel<64, false>",
                "tail_decoder": "ita_gemm_f16x3_kernel<128, 128, 2, 4>", "lstm_fc": "ita_lstm_layer_kernel<4>"}
# algorithmic HBM bytes per frame of each stage as it is cut here (inputs + outputs that cross a launch)
STAGE_BYTES = {"tokenizer": 21600 + 128 * 64 * 4, "encoder": 128 * 64 * 4 + 2 * 128 * 64 * 2,
               "tail_decoder": 2 * 128 * 64 * 2 + 512 * 4, "lstm_fc": 2 * 3 * 128 * 4 * 2 + 12}


def pmc_traffic(kernel, frames):
    try:
        with open(os.path.join(REPO, "profiles", "kernel_traffic.json")) as f:
            t = json.load(f)
        k = t["kernels"][kernel]
        return int(k["hbm_bytes_per_launch"] * frames / 1024), t["source"]
    except Exception:
        return None, None


DUMP_LIMIT = 60_000_000     # bytes of all --dump-outputs arrays together


def dump_outputs(path, arrays):
    """arrays: name -> (tensor, frame axis); written as path/<name>.npy in float32.  Beyond DUMP_LIMIT bytes in all, every
    array keeps the same fraction of its frames, chosen by a fixed seed, so that runs with the same arguments compare."""
    os.makedirs(path, exist_ok=True)
    arrays = {k: (t.detach().float().cpu().numpy(), ax) for k, (t, ax) in arrays.items()}
    keep = min(1.0, DUMP_LIMIT / sum(x.nbytes for x, _ in arrays.values()))
    for name, (x, ax) in arrays.items():
        if keep < 1.0:
            n = x.shape[ax]
            x = np.take(x, np.sort(np.random.default_rng(0).choice(n, max(1, int(n * keep)), replace=False)), axis=ax)
        np.save(os.path.join(path, name + ".npy"), np.ascontiguousarray(x, dtype=np.float32))


def _cpu_worker(job):
    blob, n, reps, seed = job
    from drone_oa_iree_vit_accelerator_amd import synth
    from oracle import oracle
    fr = synth.frames(seed, n)
    for _ in range(reps):
        oracle.forward(blob, fr["img_u8"], fr["desvel"], fr["quat"])
    return n * reps


def host_core_share():
    """host cores this command may use for the CPU baseline = the box's share for this GPU: the container's CPU quota
    (cgroup cpu.max: quota / period) when one is set, else the scheduler affinity mask.  Returned with its source."""
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = os.cpu_count() or 1
    src = "sched_getaffinity"
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            txt = open(path).read().split()
            if path.endswith("cpu.max"):
                quota, period = txt[0], float(txt[1])
            else:
                quota, period = txt[0], float(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if quota not in ("max", "-1"):
                q = int(float(quota) / period + 0.5)
                if 1 <= q < avail:
                    avail, src = q, "cgroup cpu quota"
            break
        except Exception:
            continue
    if avail > 32:      # bound the worker pool (the GPU boxes allow a command a limited number of processes)
        avail, src = 32, src + ", capped at 32"
    return max(1, avail), src


def cpu_baseline(blob, fp, target_s=8.0):
    """Two CPU figures on this box's host cores, both on a bounded sample of the same synthetic workload, both BEFORE the
    GPU is initialised in this process (the port's workers are forked):
      value / kind "torch-f32-eager": the float twin of the graph (float_twin.py: true softmax, f32 -- what the
          reference's llvm-cpu .vmfb holds; no IREE in the image, so this is SURVEY.md section 8(d) C1's stated fallback),
          PyTorch eager with `cores` intra-op threads;
      port: the int8 oracle (oracle/ita_oracle.c, scalar C), one process per core, and one core alone."""
    import concurrent.futures as cf
    import multiprocessing as mp
    import torch
    from drone_oa_iree_vit_accelerator_amd import synth
    from drone_oa_iree_vit_accelerator_amd.float_twin import FloatTwin
    from oracle import oracle
    cores, cores_src = host_core_share()
    # ---- float twin, torch eager
    torch.set_num_threads(cores)
    tw = FloatTwin(fp)
    frt = synth.frames(1234, 256)
    imgs = torch.from_numpy(frt["img_u8"])
    dvt, qtt = torch.from_numpy(frt["desvel"]), torch.from_numpy(frt["quat"])
    tw.forward(imgs[:32], dvt[:32], qtt[:32])
    t0 = time.perf_counter()
    n_tw, hidden = 0, None
    while time.perf_counter() - t0 < target_s:
        _, hidden = tw.forward(imgs, dvt, qtt, hidden)
        n_tw += imgs.shape[0]
    dt_tw = time.perf_counter() - t0
    # ---- scalar int8 port
    fr = synth.frames(1234, 64)
    t0 = time.perf_counter()
    oracle.forward(blob, fr["img_u8"][:4], fr["desvel"][:4], fr["quat"][:4])
    per = (time.perf_counter() - t0) / 4
    n = int(max(8, min(64, target_s / max(per, 1e-6))))
    reps = max(1, int(round(target_s / (per * n))))
    t0 = time.perf_counter()
    for _ in range(reps):
        oracle.forward(blob, fr["img_u8"][:n], fr["desvel"][:n], fr["quat"][:n])
    dt1 = time.perf_counter() - t0
    t0 = time.perf_counter()
    with cf.ProcessPoolExecutor(max_workers=cores, mp_context=mp.get_context("fork")) as ex:
        done = sum(ex.map(_cpu_worker, [(blob, n, reps, 1234 + w) for w in range(cores)]))
    dtm = time.perf_counter() - t0
    return {"value": round(n_tw / dt_tw, 2), "unit": "frames/s", "cores": cores, "kind": "torch-f32-eager",
            "sample": f"{n_tw} frames (batches of 256, LSTM state carried) of the same synthetic workload through the float "
                      f"twin of the graph (float_twin.py, true softmax, f32) in PyTorch {torch.__version__} eager with "
                      f"{cores} intra-op threads, {dt_tw:.1f} s wall; IREE is not in the image",
            "port": {"value": round(done / dtm, 2), "unit": "frames/s", "cores": cores, "kind": "port",
                     "sample": f"{cores} processes x {reps} x {n} frames through oracle/ita_oracle.c (scalar C int8 "
                               f"restatement, one thread per process, {dtm:.1f} s wall)",
                     "single_core_value": round(n * reps / dt1, 2), "single_core_sample_s": round(dt1, 1)},
            "host_cores_available": os.cpu_count(), "cores_source": cores_src}


def bench_c2(frames=1024, iters=50):
    """BASELINE config 2: the int8 MHA block alone (models/ITA_single_layer QAT, E = 128; E = 64 beside it) through
    ita_mha_int8: B = 1 p50 latency (host enqueue -> result) and the `frames`-frame launch against the int8 MFMA peak.
    Algorithmic ops per frame: E=128 37.75 MOP, E=64 25.17 MOP."""
    import torch
    from drone_oa_iree_vit_accelerator_amd import host, params
    out = {}
    for E, fixture, mop in ((128, "blocks_E128_seed0_B1.npz", 37.75e6), (64, "blocks_E64_seed2_B1.npz", 25.17e6)):
        d = params.load_fixture(os.path.join(REPO, "tests", "golden", fixture))
        eng = host.Engine(params.blob_from_record(d, None, E=E), device=torch.cuda.current_device())
        x = torch.randn((frames, 128, E), device="cuda")
        for _ in range(5):
            eng.mha(x)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            eng.mha(x)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / iters
        x1 = x[:1].contiguous()
        lat = []
        for _ in range(250):
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            eng.mha(x1)
            torch.cuda.synchronize()
            lat.append(time.perf_counter() - t1)
        # the same block at the accelerator's own boundary: int8 codes in, int8 codes out (ita_mha_q8) -- the form
        # SURVEY.md section 8(d) prices config 2 on (32 KiB of HBM traffic per E = 128 frame instead of 128 KiB)
        xq = torch.randint(-128, 128, (frames, 128, E), device="cuda", dtype=torch.int8)
        for _ in range(5):
            eng.mha_q8(xq)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(iters):
            eng.mha_q8(xq)
        e1.record()
        torch.cuda.synchronize()
        ms8 = e0.elapsed_time(e1) / iters
        tops, tops8 = mop * frames / ms / 1e9, mop * frames / ms8 / 1e9
        out[f"E{E}"] = {"frames": frames, "ops_per_launch": mop * frames, "peak_TOPs": 5000.0,
                        "int8_io": {"kernel": f"ita_stream_kernel<{E}, false, 0, false, true, FAST>  (FAST = this blob's six requantisation sites all pass the load-time single-rounding proof)", "entry": "ita_mha_q8",
                                    "ms_per_launch": round(ms8, 5), "frames_per_s": round(frames / ms8 * 1e3, 1),
                                    "achieved_TOPs": round(tops8, 1), "frac": round(tops8 / 5000.0, 4),
                                    "hbm_bytes_per_launch": 2 * 128 * E * frames},
                        "f32_io": {"kernel": f"ita_stream_kernel<{E}, false, 0, false, false, FAST>", "entry": "ita_mha_int8",
                                   "ms_per_launch": round(ms, 5), "frames_per_s": round(frames / ms * 1e3, 1),
                                   "achieved_TOPs": round(tops, 1), "frac": round(tops / 5000.0, 4),
                                   "hbm_bytes_per_launch": 2 * 128 * E * 4 * frames},
                        "frac": round(tops8 / 5000.0, 4),
                        "p50_latency_ms_b1": round(float(np.median(lat[50:])) * 1e3, 4)}
        eng.close()
    return {"workload": "int8 MHA block alone (ita_mha_int8): quantise, Q/K/V, QK^T, integer softmax, A.V, out_proj, "
                        "dequantise; weights resident, x (frames,128,E) f32 in HBM", "bound": "mfma", "dtype": "int8",
            "timing": f"torch events over {iters} back-to-back launches on the launch stream", **out}


def bench_c5(frames=32, out_ch=48, iters=20):
    """BASELINE config 5 on one GPU (256 frames over 8 GPUs = 32 per GPU): the fusion tail on a 64 x 128 token grid,
    E = 128, 48 conv outputs.  Both rooflines are reported; the binding one is the larger
    minimum time."""
    import torch
    from drone_oa_iree_vit_accelerator_amd import host, synth
    E, th, tw, co, B = 128, 64, 128, out_ch, frames
    c = synth.tail_large_case(0, E, th, tw, co, 1)
    eng = host.FusionTailLarge(c["conv_w"], c["conv_b"], device=torch.cuda.current_device())
    x = torch.randn((B, th * tw, E), device="cuda")
    out = torch.empty((B, co, 2 * th, 2 * tw), device="cuda")
    for _ in range(3):
        eng(x, th, tw, out=out)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        eng(x, th, tw, out=out)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / iters
    eng.close()
    flops = 2.0 * (E // 4 + E) * 9 * co * (2 * th) * (2 * tw) * B
    byts = (th * tw * E * 4 + co * 4 * th * tw * 4) * B          # f32 tokens in, f32 map out: what crosses HBM when fused
    t_mfma, t_hbm = flops / 2.5e15 * 1e3, byts / 8e12 * 1e3
    return {"workload": f"fusion tail on a 64x128 token grid, E=128, {co} conv outputs, {B} frames (ita_fusion_tail_large)",
            "kernel": "ita_tail_up_kernel (per-tap GEMM on the low-resolution tokens + f32 bilinear blend; shuffle channels as implicit GEMM)", "dtype": "f16x3", "frames": B, "ms_per_launch": round(ms, 5),
            "frames_per_s": round(B / ms * 1e3, 1),
            "mfma": {"achieved": round(flops / ms / 1e9, 2), "peak": 2500.0, "unit": "TFLOP/s", "frac": round(t_mfma / ms, 4),
                     "note": "algorithmic flops of the conv; executed MFMA work is 1.6x that (three split-precision products on a quarter of the pixels for the 128 upsampled channels)"},
            "hbm": {"achieved": round(byts / ms / 1e6, 1), "peak": 8000.0, "unit": "GB/s", "frac": round(t_hbm / ms, 4)},
            "bound": "mfma" if t_mfma >= t_hbm else "hbm",
            "timing": f"torch events over {iters} back-to-back launches on the launch stream"}


def bench_c5_mha(frames=32, seq=8192, iters=5):
    """BASELINE config 5 as it is worded (480 x 720 input, 64x patch-token blow-up): the int8 attention block on seq = 8192
    tokens per frame, E = 128 (ita_mha_long_q8: int8 codes in and out; three sweeps over the key tiles, Q K^T recomputed in each,
    logits never materialised).  Algorithmic int8 ops per frame (one Q K^T, one A.V, projections):
    2 * (2 * seq^2 * 192 + 4 * seq * 128 * 192); executed: three Q K^T."""
    import torch
    from drone_oa_iree_vit_accelerator_amd import host, params
    d = params.load_fixture(os.path.join(REPO, "tests", "golden", "blocks_E128_seed0_B1.npz"))
    eng = host.Engine(params.blob_from_record(d, None, E=128), device=torch.cuda.current_device())
    g = torch.Generator(device="cpu").manual_seed(5)
    base = torch.randn((frames, seq // 32, 128), generator=g).repeat_interleave(32, dim=1) * 18.0
    xq = (base + torch.randn((frames, seq, 128), generator=g) * 9.0).round().clamp(-128, 127).to(torch.int8).cuda()
    for _ in range(2):
        eng.mha_long_q8(xq)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        eng.mha_long_q8(xq)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / iters
    eng.close()
    ops = 2.0 * (2.0 * seq * seq * 192 + 4.0 * seq * 128 * 192) * frames
    executed = 2.0 * (4.0 * seq * seq * 192 + 4.0 * seq * 128 * 192) * frames
    return {"workload": f"int8 attention block on {seq} tokens per frame, E=128, {frames} frames (ita_mha_long_q8: int8 codes in / out)",
            "kernels": "ita_long_proj_kernel, ita_long_attn_kernel", "dtype": "int8", "frames": frames, "seq_len": seq,
            "ms_per_launch": round(ms, 4), "frames_per_s": round(frames / ms * 1e3, 1),
            "mfma": {"achieved": round(ops / ms / 1e9, 1), "peak": 5000.0, "unit": "TOP/s", "frac": round(ops / ms / 1e9 / 5000.0, 4),
                     "executed_frac": round(executed / ms / 1e9 / 5000.0, 4),
                     "note": "algorithmic ops (one Q K^T); the three-sweep integer softmax executes Q K^T three times"},
            "hbm_bytes_per_launch": int(frames * seq * (2 * 128 + 2 * 3 * 192)),
            "timing": f"torch events over {iters} back-to-back calls on the launch stream"}


def bench_vit2l(frames=1024, iters=50):
    """The reference's second graph family (models/ITA/QAT/model.py:22-87: E = 128, two encoder layers, no fusion tail,
    decoder on the flattened tokens), whole forward with carried state, from the committed fixture's weights."""
    import glob
    import torch
    from drone_oa_iree_vit_accelerator_amd import host, params, synth
    fx = sorted(glob.glob(os.path.join(REPO, "tests", "golden", "vit2l_*.npz")))
    if not fx:
        return None
    d = params.load_fixture(fx[0])
    fp = synth.float_params(int(d["meta.seed"]), E=128, num_layers=2, tail=False)
    eng = host.Engine(params.blob_from_record(d, fp, E=128, num_layers=2), device=torch.cuda.current_device(), reserve=frames)
    fr = synth.frames(11, frames)
    img, dv, qt = (torch.from_numpy(fr[k]).cuda() for k in ("img_u8", "desvel", "quat"))
    state = [(torch.zeros((3, frames, 128), device="cuda"), torch.zeros((3, frames, 128), device="cuda")) for _ in range(2)]
    vel = torch.empty((frames, 3), device="cuda")
    for i in range(10):
        eng.forward(img, dv, qt, state[i & 1], out=(vel, *state[(i + 1) & 1]))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(iters):
        eng.forward(img, dv, qt, state[i & 1], out=(vel, *state[(i + 1) & 1]))
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / iters * 1e3
    eng.close()
    # int8 ops per frame: two layers of (attention E = 128: 2 x (3 x 128 x 128 x 192 + 2 x 128 x 128 x 192 + 128 x 192 x 128) = 37.75 M,
    # FFN 128 -> 256 -> 128: 2 x 2 x 128 x 128 x 256 = 16.78 M)
    ops = 2 * (2 * (3 * 128 * 128 * 192 + 2 * 128 * 128 * 192 + 128 * 192 * 128) + 2 * 2 * 128 * 128 * 256)
    return {"workload": f"ITA two-layer E=128 graph without fusion tail (models/ITA/QAT/model.py), end-to-end forward, {frames} u8 frames, "
                        "state carried", "frames": frames, "ms_per_step": round(ms, 5), "frames_per_s": round(frames / ms * 1e3, 1),
            "kernels": "ita_tok_stream_kernel<128, true>, 2 x ita_stream_kernel<128, true, 0, false, false, FAST>, folded GEMM K = 16384, LSTM, fc",
            "int8_frac_of_step": round(ops * frames / (ms * 1e-3) / 5e15, 4),
            "timing": f"wall clock over {iters} forwards, one stream"}


def bench_small(blob, batches=(1, 128, 256), replays=60):
    """The small-batch / strong-scaling regime of BASELINE config 4 (1024 frames cut over 8 GPUs = 128 per GPU; config 3 =
    one frame): step time of the whole forward at 1, 128 and 256 frames per GPU with the schedule bench.py itself picks
    there (8 steps per HIP-graph replay on three streams), beside the same step on one stream (six launches per step)."""
    import torch
    from drone_oa_iree_vit_accelerator_amd import host, synth
    out = {}
    for B in batches:
        eng = host.Engine(blob, device=torch.cuda.current_device(), reserve=B)
        fr = synth.frames(4321, B)
        img, dv, qt = (torch.from_numpy(fr[k]).cuda() for k in ("img_u8", "desvel", "quat"))
        NG = 8
        g = eng.pipelined_steps(B, NG)
        g.img.copy_(img.unsqueeze(0).expand(NG, -1, -1, -1))
        g.desvel.copy_(dv.reshape(1, B).expand(NG, -1)); g.quat.copy_(qt.unsqueeze(0).expand(NG, -1, -1))
        for _ in range(40):
            g()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(replays):
            g()
        torch.cuda.synchronize()
        ms_graph = (time.perf_counter() - t0) / (replays * NG) * 1e3
        del g
        st = [(torch.zeros((3, B, 128), device="cuda"), torch.zeros((3, B, 128), device="cuda")) for _ in range(2)]
        vel = torch.empty((B, 3), device="cuda")
        for i in range(40):
            eng.forward(img, dv, qt, st[i & 1], out=(vel, *st[(i + 1) & 1]))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(replays * NG):
            eng.forward(img, dv, qt, st[i & 1], out=(vel, *st[(i + 1) & 1]))
        torch.cuda.synchronize()
        ms_stream = (time.perf_counter() - t0) / (replays * NG) * 1e3
        eng.close()
        out[f"b{B}"] = {"frames_per_gpu": B, "ms_per_step": round(ms_graph, 5), "frames_per_s": round(B / ms_graph * 1e3, 1),
                        "schedule": f"{NG} steps per HIP-graph replay on three streams: encoder(t+2) | folded GEMM(t+1) | LSTM + fc(t)",
                        "ms_per_step_one_stream": round(ms_stream, 5),
                        "timing": f"wall clock over {replays} replays ({replays * NG} steps) after 40 warm-up replays"}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--frames-per-gpu", type=int, default=1024, help="weak scaling: frames (independent streams) per GPU per step")
    ap.add_argument("--global-batch", type=int, default=0,
                    help="strong scaling (BASELINE config 4 as written: batch = 1024 over 1 -> 8 GPUs): this many frames per "
                         "step in all, cut into contiguous per-GPU shards (dist.shard_range); overrides --frames-per-gpu")
    ap.add_argument("--image-dtype", choices=["u8", "f32"], default="u8",
                    help="u8: the wire format of the reference host (ita_wire.h; the /255.0f of main.cpp:168-169 is folded into "
                         "the conv weights of the fused tokenizer+encoder kernel, the blend done exactly on the pixel codes); "
                         "f32: the graph's own input type (stand-alone tokenizer launch, 4x the frame bytes)")
    ap.add_argument("--settle-steps", type=int, default=int(os.environ.get("ITA_BENCH_SETTLE", "512")),
                    help="untimed steps run before the timed region in addition to --warmup, so that at least this many steps "
                         "precede it (GPU clock settle; reported as `settle_steps`)")
    ap.add_argument("--schedule", choices=["auto", "stream", "pipelined", "graph"], default="auto",
                    help="stream: one ita_vitlstm_forward per step on one stream.  pipelined: ita_vitlstm_pipelined, the "
                         "library's own two-stream loop (front(t+1) next to back(t), two host threads), 8 steps per call.  "
                         "graph: the same pipeline captured in a HIP graph (host.PipelinedSteps).  auto: graph when a GPU "
                         "gets at most 256 frames per step (the encoder then leaves CUs free for the LSTM kernels), else stream")
    ap.add_argument("--hip-graph", choices=["auto", "on", "off"], default=None,
                    help="older spelling: on = --schedule graph, off = --schedule stream")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline figure does not need: roofline and per-stage table, p50 latency, "
                         "CPU baseline, the other BASELINE configurations (each in runs of its own after the timed steps)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the velocities and LSTM state of the last timed step as DIR/<name>.npy (float32)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-latency", action="store_true")
    ap.add_argument("--no-configs", action="store_true", help="skip the BASELINE config 2 / config 5 legs (configs.c2, configs.c5)")
    ap.add_argument("--gather-every", type=int, choices=[1, 8], default=1,
                    help="N > 1: steps per velocity all-gather.  1 (default): one asynchronous all-gather per time step, the "
                         "exchange BASELINE.json's north_star names -- a consumer sees a step's velocities one step later.  "
                         "8: the velocities of 8 steps travel in one all-gather (fewer collective kernels beside the encoder's "
                         "persistent workgroups, but a consumer sees them up to 16 steps late).  The graph / pipelined schedules "
                         "replay 8 steps per host call and therefore always gather once per replay; the line says which was timed")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend (nccl = RCCL); 'gloo' only to "
                    "rehearse the N>1 code path with several ranks on one GPU (set ITA_FORCE_DEVICE=0)")
    a = ap.parse_args()

    from drone_oa_iree_vit_accelerator_amd import dist as itadist
    from drone_oa_iree_vit_accelerator_amd import params, synth
    rank, local_rank, world = itadist.env_world()
    fx = params.load_fixture(os.path.join(REPO, "tests", "golden", "vitlstm_E64_seed0_B2.npz"))
    fp0 = synth.float_params(0, E=64)
    blob = params.blob_from_record(fx, fp0, E=64)     # weights: seed 0 synthetic-QAT
    cpu = None
    if a.full and world == 1 and not a.no_cpu_baseline:      # before anything touches the GPU: the CPU workers are forked
        cpu = cpu_baseline(blob, fp0)

    import torch
    import torch.distributed as dist
    from drone_oa_iree_vit_accelerator_amd import host
    if world != a.gpus:
        if world == 1 and a.gpus > 1:
            raise SystemExit("launch N>1 with: python -m torch.distributed.run --nproc-per-node N bench.py --gpus N")
        raise SystemExit(f"--gpus {a.gpus} but WORLD_SIZE={world}")
    if "ITA_FORCE_DEVICE" in os.environ:
        local_rank = int(os.environ["ITA_FORCE_DEVICE"])
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    itadist.init(a.backend, local_rank)

    K, W = a.steps, a.warmup
    strong = a.global_batch > 0
    if strong:
        lo, hi = itadist.shard_range(a.global_batch, rank, world)
        B, total = hi - lo, a.global_batch
        if B == 0:
            raise SystemExit("--global-batch smaller than the number of GPUs")
    else:
        B, total, lo = a.frames_per_gpu, a.frames_per_gpu * world, a.frames_per_gpu * rank
    eng = host.Engine(blob, device=local_rank, reserve=B)
    fr = synth.frames(1234 + rank, B)
    if a.image_dtype == "u8":
        img = torch.from_numpy(fr["img_u8"]).to(dev)
    else:
        # the reference host's float(pixel) / 255.0f (main.cpp:168-169), IEEE division on the CPU
        img = torch.from_numpy(fr["img_u8"].astype(np.float32) / np.float32(255.0)).to(dev)
    dv, qt = torch.from_numpy(fr["desvel"]).to(dev), torch.from_numpy(fr["quat"]).to(dev)
    state = [(torch.zeros((3, B, 128), device=dev), torch.zeros((3, B, 128), device=dev)) for _ in range(2)]
    vels = [torch.empty((B, 3), device=dev) for _ in range(3)]
    gather = itadist.VelocityGather(B, world, dev, total=total if strong else None)
    NG = 8                                        # time steps per graph replay
    sched = {"on": "graph", "off": "stream"}.get(a.hip_graph, a.schedule)
    if sched == "auto":
        # measured (tools/pipeline_probe.py, tools/pipeline3_probe.py, bench --schedule ...): the three-stage graph replay
        # gives 38 us per step at 128 frames and 48 at 256, the library's two-stage two-thread loop 44 / 50; below that the
        # graph wins (the step is launch-bound and a replay has no launches)
        # (at 512 / 1024 frames the graph replay is also 3 % / 2 % faster than one stream, but the dominant kernel's launch
        #  time for the roofline is then not measured inside the timed region: the default stays "stream" there)
        sched = "stream" if (B > 256 or a.image_dtype != "u8" or K % NG) else "graph"
    if sched == "pipelined" and K % 40 == 0:
        NG = 40        # steps per ita_vitlstm_pipelined call: the helper thread is started once per call
    if sched != "stream" and (a.image_dtype != "u8" or K % NG):
        raise SystemExit(f"--schedule {sched} needs u8 frames and --steps that is a multiple of {NG}")
    graph = None
    if sched == "graph":
        # NG steps per replay on three streams, encoder(t+2) | folded GEMM(t+1) | LSTM + fc(t): host.PipelinedSteps
        graph = eng.pipelined_steps(B, NG)
        graph.img.copy_(img.unsqueeze(0).expand(NG, -1, -1, -1))
        graph.desvel.copy_(dv.reshape(1, B).expand(NG, -1)); graph.quat.copy_(qt.unsqueeze(0).expand(NG, -1, -1))
    elif sched == "pipelined":
        class LibPipeline:
            """NG steps per ita_vitlstm_pipelined call; same calling convention as host.PipelinedSteps here"""
            def __init__(self):
                self.vel = torch.empty((NG, B, 3), device=dev)
                self.h, self.c = state[0]
                self.sf, self.sb = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
                self.args = ([img] * NG, [dv.reshape(B)] * NG, [qt] * NG, (self.h, self.c), [self.vel[i] for i in range(NG)])

            def __call__(self):
                eng.pipelined(*self.args, self.sf, self.sb)     # joins on its front stream: run under torch.cuda.stream(sf)
        graph = LibPipeline()
    batched_gather = graph is None and a.gather_every == NG
    velring = torch.empty((2, NG, B, 3), device=dev) if batched_gather else None
    gather_every = NG if (graph is not None or batched_gather) else 1
    if gather_every == NG:
        # one all-gather per NG steps: rank r sends NG x (its shard) rows; uneven shards (strong scaling) are padded to the
        # longest.  A graph replay / library call writes ONE velocity buffer again and again, so its rows are staged into
        # the gather's own ping-pong send buffers (stream-ordered copy) before the collective starts.
        shard = [hi_ - lo_ for lo_, hi_ in (itadist.shard_range(total, r, world) for r in range(world))] if strong else [B] * world
        gather = itadist.VelocityGather(NG * B, world, dev, sizes=[NG * sz for sz in shard], stage=graph is not None)
    torch.cuda.synchronize()

    def step(i):
        """one time step over this GPU's B streams (+ the asynchronous velocity all-gather for N > 1)"""
        if graph is not None:
            if i % NG == 0:       # a replay / call covers steps i .. i + NG - 1
                # (the library pipeline's calls and their all-gathers stay on its front stream: no join with another
                #  stream between calls, the next call's fronts queue up behind this call's last back)
                with torch.cuda.stream(graph.sf) if sched == "pipelined" else contextlib.nullcontext():
                    graph()      # (its one velocity buffer is free: gather.start staged the previous replay's rows)
                    if world > 1:
                        gather.start(graph.vel.reshape(NG * B, 3))
            return
        src, dst = state[i & 1], state[(i + 1) & 1]
        if batched_gather:
            # --gather-every 8: the velocities of NG steps go out in ONE all-gather (96 KiB instead of eight times 12 KiB).
            # The encoder's persistent workgroups need every CU; a collective's kernel that holds one for 10-20 us delays
            # the whole launch by that much, so the fewer collectives share the GPU with it the better.
            half, k = (i // NG) & 1, i % NG
            if world > 1 and k == 0:
                gather.ready()      # the all-gather of two groups ago read this half of the velocity ring
            eng.forward(img, dv, qt, src, out=(velring[half][k], dst[0], dst[1]))
            if world > 1 and k == NG - 1:
                gather.start(velring[half].reshape(NG * B, 3))
            return
        vel = vels[i % 3]
        if world == 1:
            eng.forward(img, dv, qt, src, out=(vel, dst[0], dst[1]))
            return
        # N > 1, one all-gather per step.  The collective of step i - 1 is enqueued BEHIND this step's encoder: issued right after
        # fc(i - 1) its kernel becomes runnable in the same instant as the encoder, whose 256 persistent workgroups need every CU --
        # when the collective wins that race the encoder's last workgroup starts 10-20 us late and the step is that much longer.
        # Behind the encoder it runs beside the folded GEMM (128 KB of LDS and four waves per CU leave it room).  Same kernels and
        # arithmetic as eng.forward (ita_vitlstm_encode / _fold / _back on one stream); three velocity buffers, because the
        # all-gather that read buffer i % 3 is the one started two starts ago -- what gather.ready() waits for.
        gather.ready()
        eng.encode(img, i & 1)
        if pending[0] is not None:
            gather.start(pending[0])
        eng.fold(B, i & 1, i % 3)
        eng.back(dv, qt, src, (vel, dst[0], dst[1]), i % 3)
        pending[0] = vel

    pending = [None]      # the velocity buffer whose all-gather has not been started yet (N > 1, per-step gather)

    def flush():
        if pending[0] is not None:
            gather.start(pending[0])
            pending[0] = None
        gather.finish()

    def fence():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    for i in range(W if graph is None else -(-W // NG) * NG):   # graph schedule: whole replays (>= W steps)
        step(i)
    flush()
    fence()
    # Clock settle: a short run (the driver's --steps 20 --warmup 5 is 2.7 ms of GPU work) is over before the GPU's power
    # management has settled under load (measured on MI355X boxes: the same kernels run 6 % slower in the first few ms after
    # idle than after 30 ms of load).  These steps are untimed and in addition to the W warmup steps.
    settle = max(0, a.settle_steps - W) // NG * NG
    for i in range(settle):
        step(i)
    flush()
    fence()
    # u8 wire frames: the tokenizer runs inside the encoder kernel (ita_stream_kernel<64, true, 1>), one stage;
    # f32 frames go through the stand-alone tokenizer launch
    fused_tok = not os.environ.get("ITA_SPLIT_TOKENIZER") and a.image_dtype == "u8"
    if a.full:
        # Untimed eager pass with HIP events around EVERY stage: the per-stage table and the dominant stage.
        # (Each event costs a ~5 us bubble in the stream, so this pass is slower than the timed one.)
        NP = 20
        eng.profile_begin(NP)
        for i in range(NP):
            src, dst = state[(W + i) & 1], state[(W + i + 1) & 1]
            eng.forward(img, dv, qt, src, out=(vels[0], dst[0], dst[1]))
        fence()
        stage_all, n_all = eng.profile_end()
        per = {k: v / max(n_all, 1) for k, v in stage_all.items()}
        per["tail_decoder"] = per.pop("tail") + per.pop("decoder")
        per["encoder"] = per.pop("mha") + per.pop("ffn")
        if fused_tok:
            per["encoder"] += per.pop("tokenizer")
        dom = max(per, key=per.get)
        dom_plugin_stage = {"encoder": "mha", "tail_decoder": "tail", "lstm_fc": "lstm_fc", "tokenizer": "tokenizer"}[dom]
    # Timed region: exactly K steps.  With --full, eager schedule: HIP events around the dominant kernel only, on every 8th
    # step (its launch duration for the roofline is measured here, live, on the compute stream).  Pipelined / graph schedules:
    # no timing events inside, so the dominant kernel is timed the same way in an eager pass right after the timed region.
    live = a.full and graph is None and not os.environ.get("ITA_BENCH_NOPROF")
    if live:
        eng.profile_begin(min(K, 512), every_n=8, only_stage=dom_plugin_stage)
    t0 = time.perf_counter()
    for i in range(K):
        step(i)
    flush()
    fence()
    elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed], device=dev if a.backend == "nccl" else "cpu", dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    if a.dump_outputs and rank == 0:
        # what step K - 1 handed its caller, taken before --full's passes below reuse these buffers
        if graph is not None:           # one replay / library call = NG steps; its last step wrote vel[NG - 1]
            vel, (h, c) = graph.vel[NG - 1], (graph.h, graph.c)
        elif batched_gather:
            vel, (h, c) = velring[((K - 1) // NG) & 1][(K - 1) % NG], state[K & 1]
        else:
            vel, (h, c) = vels[(K - 1) % 3], state[K & 1]
        if world > 1:                   # the caller's velocities are those of every GPU: the last all-gather started
            vel = gather.result(gather.i ^ 1)
            if gather_every == NG:      # each rank sent NG steps x its shard: keep every rank's last step
                vel = torch.cat([r.reshape(NG, -1, 3)[NG - 1] for r in torch.split(vel, gather.sizes)])
        dump_outputs(a.dump_outputs, {"velocity": (vel, 0), "h": (h, 1), "c": (c, 1)})
    if a.full:
        if live:
            stage_ms, nprof = eng.profile_end()
            timing = "HIP events around this kernel on every 8th step of the timed region"
        else:
            eng.profile_begin(64, every_n=2, only_stage=dom_plugin_stage)
            for i in range(128):
                src, dst = state[i & 1], state[(i + 1) & 1]
                eng.forward(img, dv, qt, src, out=(vels[0], dst[0], dst[1]))
            fence()
            stage_ms, nprof = eng.profile_end()
            timing = ("HIP events around this kernel on every 2nd step of a 128-step eager pass right after the timed region "
                      "(the timed region replays HIP graphs, which cannot carry timing events)")
        dom_ms = stage_ms[dom_plugin_stage] / max(nprof, 1)

    out = None
    if rank == 0:
        frames_per_step = total
        wl = (f"{a.global_batch} synthetic 60x90 depth frames per step in all, contiguous shards over {world} GPU(s)" if strong
              else f"{B} synthetic 60x90 depth frames per GPU per step")
        out = {
            "metric": "frames/s on ITAViTLSTM int8, 60x90 depth input",
            "value": round(frames_per_step * K / elapsed, 1), "unit": "frames/s", "n_gpus": world, "steps": K, "warmup": W, "settle_steps": settle,
            "ms_per_step": round(elapsed / K * 1e3, 5), "higher_is_better": True, "scaling": "strong" if strong else "weak",
            "vs_baseline": None, "dtype": "int8+f32", "data": "synthetic",
            "config": {"workload": "ITAViTLSTM int8 end-to-end forward (BASELINE config 4): " + wl +
                                   ", LSTM state carried, velocity all-gather",
                       "frames_per_gpu": B, "global_batch": frames_per_step, "parallelism": f"dp{world}",
                       "image_dtype": a.image_dtype, "weights": "seed-0 synthetic QAT (tests/golden)",
                       "gather_every": gather_every,
                       "gather": ("none (one GPU)" if world == 1 else
                                  f"asynchronous all-gather of the (frames, 3) velocities every {gather_every} step(s), "
                                  f"double-buffered, backend {a.backend}"
                                  + (", each enqueued behind the next step's encoder launch (it runs beside the folded GEMM, not "
                                     "in a race with the encoder's 256 persistent workgroups for CUs)" if gather_every == 1 and graph is None else "")),
                       "schedule": {"stream": "one stream",
                                    "graph": f"{NG} steps per HIP-graph replay on three streams: encoder(t+2) | folded GEMM(t+1) | LSTM + fc(t)",
                                    "pipelined": f"{NG} steps per ita_vitlstm_pipelined call: the library's two-stream loop, "
                                                 "front(t+1) overlaps back(t)"}[sched]},
        }
    if rank == 0 and a.full:
        ops, bound, peak, arith = STAGE_WORK[dom]
        if nprof == 0:
            dom_ms = per[dom]
        achieved = ops * B / (max(dom_ms, 1e-9) * 1e-3) / 1e12
        kname = STAGE_KERNEL.get(dom, dom)
        if dom == "encoder":
            # (last template argument: the single-rounding requantisation form -- the seed-0 blob passes the load-time proof)
            kname = "ita_stream_kernel<64, true, 1, false, false, true>" if fused_tok else "ita_stream_kernel<64, true, 0, false, false, true>"
        traffic, tsrc = pmc_traffic(kname, B)
        roof = {"kernel": kname, "stage": dom, "bound": bound, "achieved": round(achieved, 3),
                "peak": peak, "unit": "TFLOP/s", "frac": round(achieved / peak, 5), "traffic": traffic,
                "traffic_source": tsrc, "kernel_cut_hbm_bytes_per_launch": STAGE_BYTES.get(dom, 0) * B,
                "arithmetic": arith, "ops_per_launch": ops * B, "avg_launch_ms": round(dom_ms, 5),
                "launches_timed": nprof, "timing": timing}
        if dom == "encoder" and fused_tok:
            # the launch also carries the tokenizer of every frame (since round 3 its conv7x7 runs on int8 MFMA as well:
            # 23-bit fixed-point weights, six byte-plane MFMAs per 16-channel tile); `achieved` / `frac` count the int8 ops of
            # the attention and FFN blocks only (conservative, and comparable with rounds 1 and 2).  with_tokenizer adds the
            # conv's algorithmic 2 x 4.23 M ops per frame at the same peak.
            tok_ops = 2 * 4.23e6 * B
            t_min = (ops * B + tok_ops) / (peak * 1e12)
            roof["kernel_cut_hbm_bytes_per_launch"] = (5400 + 2 * 128 * 64 * 2) * B   # wire frame in, f16 hi/lo planes out
            roof["note"] = ("kernel = tokenizer (integer blend, conv on int8 MFMA) + int8 MHA + int8 FFN + three LayerNorms of each "
                            "frame; achieved/frac count the int8 ops of MHA + FFN only")
            roof["with_tokenizer"] = {"ops_per_launch": ops * B + tok_ops, "min_time_ms": round(t_min * 1e3, 5),
                                      "frac": round(t_min / (max(dom_ms, 1e-9) * 1e-3), 5)}
        # algorithmic HBM bytes of the whole step per frame with u8 ingest -- wire frame, desvel + quat,
        # (h, c) in and out, velocity out; everything between the kernels is the implementation's own traffic
        alg_step = ((5400 if a.image_dtype == "u8" else 21600) + 20 + 2 * 2 * 3 * 128 * 4 + 12) * B
        roof["step_algorithmic_hbm_bytes"] = alg_step
        stages = {}
        for k, ms in per.items():
            if k not in STAGE_WORK:
                continue
            o, _, pk, ar = STAGE_WORK[k]
            ach = o * B / (ms * 1e-3) / 1e12 if ms > 0 else 0.0
            stages[k] = {"ms": round(ms, 5), "achieved_Tops": round(ach, 3), "peak_Tops": pk, "frac": round(ach / pk, 5),
                         "arithmetic": ar}
        out.update({
            "roofline": roof, "stages": stages,
            "stages_note": "per-stage times from an untimed 20-step eager pass with events around every stage (each event "
                           "costs a ~5 us stream bubble, so they sum to more than ms_per_step)",
        })
        if not a.no_latency:      # p50 single-frame latency, host enqueue -> result ready
            e1 = host.Engine(blob, device=local_rank)
            i1, d1, q1 = img[:1].contiguous(), dv[:1].contiguous(), qt[:1].contiguous()
            st = (torch.zeros((3, 1, 128), device=dev), torch.zeros((3, 1, 128), device=dev))
            lat = []
            for it in range(250):
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                v1, st = e1.forward(i1, d1, q1, st)
                torch.cuda.synchronize()
                lat.append(time.perf_counter() - t1)
            out["p50_latency_ms_b1"] = round(float(np.median(lat[50:])) * 1e3, 4)
            if a.image_dtype == "u8":
                # the same step replayed from a HIP graph (six launches -> one host call), in-place state
                g1 = e1.graphed_step(1)
                g1.img.copy_(i1); g1.desvel.copy_(d1.reshape(1)); g1.quat.copy_(q1)
                lat = []
                for it in range(250):
                    torch.cuda.synchronize()
                    t1 = time.perf_counter()
                    g1()
                    torch.cuda.synchronize()
                    lat.append(time.perf_counter() - t1)
                out["p50_latency_ms_b1_hipgraph"] = round(float(np.median(lat[50:])) * 1e3, 4)
                del g1
            e1.close()
        out["cpu_baseline"] = cpu
        if world == 1 and not a.no_configs:
            # the other single-GPU configurations of BASELINE.json, measured in this same run
            del graph
            eng.close()
            out["configs"] = {"c2": bench_c2(), "c5": bench_c5(), "c5_mha": bench_c5_mha(), **bench_small(blob)}
            v2 = bench_vit2l()
            if v2:
                out["configs"]["vit2l"] = v2
    fence()
    if rank == 0:
        print(json.dumps(out), flush=True)
    eng.close()
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
