#!/usr/bin/env python3
"""Step time of the float ViT+LSTM graph (models/ITA_single_layer_upsample_shuffle/model.py: float32 attention with a
true softmax, float32 FFN, nothing quantised; an ITAW0003 blob) on the GPU box.  Prints one JSON line: ms per step and
frames/s at 1024 and at 128 frames, the single-frame p50 latency, and the kernel labels.  For the kernel time of
ita_attn_f32_kernel<E> run it under rocprofv3 --kernel-trace --stats (a run of its own).
--E 128: the E = 128 float graph without the fusion tail (models/ITA_upsample_shuffle/model.py, run it with --layers 2):
ita_attn_f32_kernel<128> and ita_ffn_f32_kernel<128>, decoder 16384 -> 512 on the flattened tokens.
usage: python tools/bench_float.py [--E 64|128] [--layers 1|2] [--steps K]"""
import argparse, json, os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from drone_oa_iree_vit_accelerator_amd import host, params, synth

ap = argparse.ArgumentParser()
ap.add_argument("--layers", type=int, default=1, choices=(1, 2))
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--E", type=int, default=64, choices=(64, 128))
a = ap.parse_args()
blob = params.blob_from_float_params(synth.float_params(0, E=a.E, num_layers=a.layers, tail=a.E == 64), a.layers)


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
if a.E == 64:
    graph = f"float ITALSTMNetVIT E=64 {a.layers} layer(s)"
    kernels = ["ita_tok_stream_kernel<64,true>", "ita_attn_f32_kernel<64> (attention + LN1, f32 MFMA)",
               "ita_ffn_f32_kernel<64> (FFN + LN2, f32 MFMA)", "ita_gemm_f16x3_kernel (folded tail+decoder)"]
else:
    graph = f"float ITALSTMNetVIT E=128 {a.layers} layer(s), no fusion tail (ITA_upsample_shuffle)"
    kernels = ["ita_tok_stream_kernel<128,true>", "ita_attn_f32_kernel<128> (attention + LN1, f32 MFMA)",
               "ita_ffn_f32_kernel<128> (FFN + LN2, f32 MFMA)", "ita_gemm_f16x3_kernel (folded decoder, K = 16384)"]
print(json.dumps({"graph": graph, "ms_per_step_1024": round(ms1024, 4),
                  "frames_per_s_1024": round(1024 / ms1024 * 1e3), "ms_per_step_128": round(ms128, 4),
                  "frames_per_s_128": round(128 / ms128 * 1e3), "p50_ms_1frame": round(p50, 4),
                  "kernels": kernels + ["ita_lstm_head_kernel"]}))
