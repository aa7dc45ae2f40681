#!/usr/bin/env python3
"""Cost of the float graph on long sequences (GPU box): S = 8192 tokens per frame, 32 frames, ITAW0003 blobs at E = 64
(one layer, with the fusion tail) and E = 128 (two layers).

  mha_long_f32   ita_mha_long_f32: the projection launch (K / V fragment images to the workspace) and the one-sweep
                 running-softmax attention launch
  layer          ita_encoder_layer_long_f32: those two launches with residual + LayerNorm1, then the float FFN kernel
                 with residual + LayerNorm2 in place
  chain          token rows -> encode_long_f32 (all layers) -> ita_fusion_tail_large on the 64 x 128 token grid, 48 outputs
  torch          FloatTwin(..., device="cuda")._attention on the same GPU: torch's GEMMs and softmax, which materialise
                 the (frames, S, S) logits -- 268 MB per frame at S = 8192, so it runs on --torch-frames frames (default 4)
                 and is compared per frame

Comparators per figure: floor_fraction = the f32-MFMA floor of the two attention sweeps, 2 x 2 x B x S^2 x 192 flop at
157.3 TF (10.5 ms at 32 x 8192, once per layer), over the measured time; ratio_to_torch = torch's time per frame over this
path's time per frame (mha_long_f32 only).

Device events around --launches calls after a warm-up, --rounds rounds with the figures interleaved; min / median / max
per figure.  usage: python tools/bench_long_f32.py [--out profiles/long_f32.json] [--frames 32] [--seq 8192]
[--launches 3] [--rounds 5] [--torch-frames 4]"""
import argparse, json, os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from drone_oa_iree_vit_accelerator_amd import float_twin, host, params, synth

F32_MFMA_FLOPS = 157.3e12
LAYERS = {64: 1, 128: 2}


def timed_us(fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / launches


def stats(v):
    return {"min": round(min(v), 1), "median": round(float(np.median(v)), 1), "max": round(max(v), 1), "rounds": [round(x, 1) for x in v]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--seq", type=int, default=8192)
    ap.add_argument("--launches", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--torch-frames", type=int, default=4)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_long_f32.py measures on the GPU: none visible")
    B, S, Bt, lib = a.frames, a.seq, min(a.torch_frames, a.frames), host.lib()
    th, tw, co = 64, S // 64, 48
    floor_us = 2 * 2 * B * S * S * 192 / F32_MFMA_FLOPS * 1e6
    fns, sweeps, keep = {}, {}, []
    for E in (128, 64):
        L = LAYERS[E]
        fp = synth.float_params(E, E=E, num_layers=L, tail=(E == 64))
        eng = host.Engine(params.blob_from_float_params(fp, L), device=0)
        twin = float_twin.FloatTwin(fp, num_layers=L, device="cuda")
        g = torch.Generator(device="cpu").manual_seed(5 + E)      # LayerNorm-like rows, as the tests build them
        x = torch.randn((B, S, E), generator=g)
        x = ((x - x.mean(-1, keepdim=True)) / x.std(-1, keepdim=True, unbiased=False)).cuda()
        y = torch.empty_like(x)
        sp = host._stream_ptr(0)
        c = synth.tail_large_case(0, E, th, tw, co, 1)
        tail = host.FusionTailLarge(c["conv_w"], c["conv_b"], device=0)
        fmap = torch.empty((B, co, 2 * th, 2 * tw), device="cuda")
        keep.append((eng, x, y, twin, tail, fmap))

        def mha(eng=eng, x=x, y=y, sp=sp):
            host._chk(lib.ita_mha_long_f32(eng._h, 0, x.data_ptr(), y.data_ptr(), B, S, sp))

        def layer(eng=eng, x=x, y=y):
            eng.encoder_layer_long_f32(x, 0, out=y)

        def chain(eng=eng, x=x, tail=tail, fmap=fmap):
            tail(eng.encode_long_f32(x), th, tw, out=fmap)

        def torch_attn(twin=twin, x=x):
            with torch.no_grad():
                twin._attention(x[:Bt], 0)

        fns.update({f"mha_long_f32_E{E}": mha, f"layer_E{E}": layer, f"chain_E{E}": chain, f"torch_attention_E{E}": torch_attn})
        sweeps.update({f"mha_long_f32_E{E}": 1, f"layer_E{E}": 1, f"chain_E{E}": L})
    for f in fns.values():
        for _ in range(2):
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(a.rounds):
        for k, f in fns.items():       # interleaved: a drift of the box moves every figure alike
            t[k].append(timed_us(f, a.launches))
    figures = {}
    for k, v in t.items():
        med = float(np.median(v))
        fig = dict(stats(v))
        if k in sweeps:
            fig["floor_us"] = round(floor_us * sweeps[k], 1)
            fig["floor_fraction"] = round(floor_us * sweeps[k] / med, 3)
            fig["frames_per_s"] = round(B / med * 1e6, 1)
        else:
            fig["frames"] = Bt
        if k.startswith("mha_long_f32_E"):
            tt = float(np.median(t["torch_attention_E" + k.rsplit("E", 1)[1]]))
            fig["ratio_to_torch"] = round((tt / Bt) / (med / B), 2)
        figures[k] = fig
    res = {"tool": "tools/bench_long_f32.py", "device": torch.cuda.get_device_name(0), "frames": B, "seq_len": S,
           "torch_frames": Bt, "launches_per_round": a.launches, "rounds": a.rounds, "unit": "us per call",
           "blobs": {"E64": "synth.float_params(64, E=64), one layer, ITAW0003", "E128": "synth.float_params(128, E=128, num_layers=2, tail=False), ITAW0003"},
           "floor": "2 * 2 * frames * seq_len^2 * 192 flop per layer at 157.3 TF (f32 MFMA)", "figures": figures}
    for item in keep:
        item[0].close()
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
