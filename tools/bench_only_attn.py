#!/usr/bin/env python3
"""Step time of the attention-only QAT graph (models/ITA_single_layer_upsample_shuffle/QAT_only_attn/model.py: int8
attention, float32 FFN + residual + LayerNorm2; an ITAW0002 blob) on the GPU box.  Prints one JSON line: ms per step
and frames/s at 1024 and at 128 frames, the single-frame p50 latency, and the kernel labels.  For the kernel time of
ita_ffn_f32_kernel<64> run it under rocprofv3 --kernel-trace --stats (a run of its own).
usage: python tools/bench_only_attn.py [--layers 1|2] [--steps K]"""
import argparse, glob, json, os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from drone_oa_iree_vit_accelerator_amd import host, params, synth

ap = argparse.ArgumentParser()
ap.add_argument("--layers", type=int, default=1, choices=(1, 2))
ap.add_argument("--steps", type=int, default=100)
a = ap.parse_args()
path = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden",
                                     f"onlyattn{a.layers}l_E64_*.npz")))[0]
d = params.load_fixture(path)
fp = synth.float_params(int(d["meta.seed"]), E=64, num_layers=a.layers)
blob = params.blob_from_record(d, fp, E=64, num_layers=a.layers)


def step_ms(B, K):
    eng = host.Engine(blob, device=0, reserve=B)
    fr = synth.frames(11, B)
    img, dv, qt = (torch.from_numpy(fr[k]).cuda() for k in ("img_u8", "desvel", "quat"))
    state = [(torch.zeros((3, B, 128), device="cuda"), torch.zeros((3, B, 128), device="cuda")) for _ in range(2)]
    vel = torch.empty((B, 3), device="cuda")
    for i in range(20):
        eng.forward(img, dv, qt, state[i & 1], out=(vel, *state[(i + 1) & 1]))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(K):
        eng.forward(img, dv, qt, state[i & 1], out=(vel, *state[(i + 1) & 1]))
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / K
    lat = []
    if B == 1:
        for i in range(K):
            t0 = time.perf_counter()
            eng.forward(img, dv, qt, state[i & 1], out=(vel, *state[(i + 1) & 1]))
            torch.cuda.synchronize()
            lat.append(time.perf_counter() - t0)
    eng.close()
    return dt * 1e3, (float(np.percentile(lat, 50)) * 1e3 if lat else None)


ms1024, _ = step_ms(1024, a.steps)
ms128, _ = step_ms(128, a.steps)
_, p50 = step_ms(1, a.steps)
print(json.dumps({"graph": f"QAT_only_attn E=64 {a.layers} layer(s)", "ms_per_step_1024": round(ms1024, 4),
                  "frames_per_s_1024": round(1024 / ms1024 * 1e3), "ms_per_step_128": round(ms128, 4),
                  "frames_per_s_128": round(128 / ms128 * 1e3), "p50_ms_1frame": round(p50, 4),
                  "kernels": ["ita_tok_stream_kernel<64,true>", "ita_stream_kernel<64,false,0,false,false,*> (attention + LN1)",
                              "ita_ffn_f32_kernel<64> (FFN + LN2, f32 MFMA)", "ita_gemm_f16x3_kernel (folded tail+decoder)",
                              "ita_lstm_head_kernel"]}))
