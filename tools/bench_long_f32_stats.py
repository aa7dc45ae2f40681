#!/usr/bin/env python3
"""Cost of the long float statistics (GPU box): 32 frames of S = 8192 tokens, the ITAW0003 blobs and inputs of
tools/bench_long_f32.py at E = 64 and E = 128.

  mha_long_f32  ita_mha_long_f32 of this build: projection launch + one sweep of Q K^T, running softmax and P V + out_proj
  stats_all     ita_mha_long_f32_stats with all six outputs: the same projection launch, two sweeps of Q K^T (the second
                forms p and reduces it along rows and columns), the reduction of the query tiles' column partials
  stats_cols    the same with col_mass and col_nnz alone
  stats_rows    the same with the four row arrays alone (no column partials, no reduction launch)

Both sides run in one process on one box, after a warm-up, --rounds rounds with the figures interleaved so that a drift
of the box moves every figure alike; device events around --launches calls.  Per figure min / median / max and every
round; per statistics figure the ratio of medians to mha_long_f32 and the ratios of the extremes (min / max, max / min).
usage: python tools/bench_long_f32_stats.py [--out profiles/long_f32_stats.json] [--frames 32] [--seq 8192]
[--launches 3] [--rounds 7]"""
import argparse, ctypes as C, json, os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from drone_oa_iree_vit_accelerator_amd import host, params, synth
from bench_long_f32 import LAYERS, stats, timed_us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--seq", type=int, default=8192)
    ap.add_argument("--launches", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_long_f32_stats.py measures on the GPU: none visible")
    B, S, lib = a.frames, a.seq, host.lib()
    fns, written, keep = {}, {}, []
    for E in (128, 64):
        L = LAYERS[E]
        fp = synth.float_params(E, E=E, num_layers=L, tail=(E == 64))
        eng = host.Engine(params.blob_from_float_params(fp, L), device=0)
        g = torch.Generator(device="cpu").manual_seed(5 + E)      # LayerNorm-like rows, as bench_long_f32.py builds them
        x = torch.randn((B, S, E), generator=g)
        x = ((x - x.mean(-1, keepdim=True)) / x.std(-1, keepdim=True, unbiased=False)).cuda()
        y, sp = torch.empty_like(x), host._stream_ptr(0)
        out = {k: torch.empty((B, S), dtype=torch.int32 if k.endswith("_nnz") else torch.float32, device="cuda")
               for k in host.LONG_F32_STATS}
        keep.append((eng, x, y, out))

        def mha(eng=eng, x=x, y=y, sp=sp):
            host._chk(lib.ita_mha_long_f32(eng._h, 0, x.data_ptr(), y.data_ptr(), B, S, sp))

        def st(names, eng=eng, x=x, out=out, sp=sp):
            s = host._MhaLongF32Stats(**{k: out[k].data_ptr() for k in names})
            keep.append((s,))
            return lambda: host._chk(lib.ita_mha_long_f32_stats(eng._h, 0, x.data_ptr(), B, S, 1.0 / 256, C.byref(s), sp))

        rows, cols = host.LONG_F32_STATS[:4], host.LONG_F32_STATS[4:]
        part = B * (S // 128) * S * 4          # one array of column partials: written once, read once
        for key, f, w in ((f"mha_long_f32_E{E}", mha, B * S * E * 4), (f"stats_all_E{E}", st(host.LONG_F32_STATS), B * S * 24 + 2 * part),
                          (f"stats_cols_E{E}", st(cols), B * S * 8 + 2 * part), (f"stats_rows_E{E}", st(rows), B * S * 16)):
            fns[key], written[key] = f, w
    for f in fns.values():
        for _ in range(2):
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(a.rounds):
        for k, f in fns.items():
            t[k].append(timed_us(f, a.launches))
    figures = {}
    for k, v in t.items():
        fig = {**stats(v), "bytes_written": written[k]}
        if k.startswith("stats_"):
            base = t["mha_long_f32_E" + k.rsplit("_E", 1)[1]]
            fig["ratio_to_mha_long_f32"] = {"of_medians": round(float(np.median(v)) / float(np.median(base)), 3),
                                            "lowest": round(min(v) / max(base), 3), "highest": round(max(v) / min(base), 3)}
        figures[k] = fig
    res = {"tool": "tools/bench_long_f32_stats.py", "device": torch.cuda.get_device_name(0), "frames": B, "seq_len": S,
           "launches_per_round": a.launches, "rounds": a.rounds, "unit": "us per call", "p_min": 1.0 / 256,
           "blobs": {"E64": "synth.float_params(64, E=64), one layer, ITAW0003", "E128": "synth.float_params(128, E=128, num_layers=2, tail=False), ITAW0003"},
           "figures": figures}
    for item in keep:
        if hasattr(item[0], "close"):
            item[0].close()
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
