#!/usr/bin/env python3
"""Cost of the long float propagation (GPU box): 32 frames of S = 8192 tokens, the ITAW0003 blobs and inputs of
tools/bench_long_f32.py at E = 64 and E = 128.

  mha_long_f32   ita_mha_long_f32 of this build: projection launch + one sweep of Q K^T, running softmax and P V + out_proj
  stats_cols     ita_mha_long_f32_stats with col_mass and col_nnz: projection, two sweeps of Q K^T, the partials' reduction
  propagate_R    ita_mha_long_f32_propagate with R = 1, 16, 64 weight rows: the K / Q projection launch, the statistics
                 kernel's sweep 1 (row maximum and row sum), the transposed sweep with a second MFMA per 16 rows

All figures run in one process on one box, after a warm-up, --rounds rounds with the figures interleaved so that a drift
of the box moves every figure alike; device events around --launches calls.  Per figure min / median / max and every
round; per propagate figure the ratio of medians to mha_long_f32 and to stats_cols and the ratios of the extremes.  There
is no pass / fail threshold.
usage: python tools/bench_long_f32_propagate.py [--out profiles/long_f32_propagate.json] [--frames 32] [--seq 8192]
[--launches 3] [--rounds 7]"""
import argparse, ctypes as C, json, os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from drone_oa_iree_vit_accelerator_amd import host, params, synth
from bench_long_f32 import LAYERS, stats, timed_us

ROWS = (1, 16, 64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--seq", type=int, default=8192)
    ap.add_argument("--launches", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_long_f32_propagate.py measures on the GPU: none visible")
    B, S, lib = a.frames, a.seq, host.lib()
    fns, keep = {}, []
    for E in (128, 64):
        L = LAYERS[E]
        fp = synth.float_params(E, E=E, num_layers=L, tail=(E == 64))
        eng = host.Engine(params.blob_from_float_params(fp, L), device=0)
        g = torch.Generator(device="cpu").manual_seed(5 + E)      # LayerNorm-like rows, as bench_long_f32.py builds them
        x = torch.randn((B, S, E), generator=g)
        x = ((x - x.mean(-1, keepdim=True)) / x.std(-1, keepdim=True, unbiased=False)).cuda()
        y, sp = torch.empty_like(x), host._stream_ptr(0)
        col = {k: torch.empty((B, S), dtype=torch.int32 if k.endswith("_nnz") else torch.float32, device="cuda")
               for k in host.LONG_F32_STATS[4:]}
        w = torch.randn((B, max(ROWS), S), generator=g).cuda()
        out = torch.empty((B, max(ROWS), S), dtype=torch.float32, device="cuda")
        st = host._MhaLongF32Stats(**{k: v.data_ptr() for k, v in col.items()})
        keep.append((eng, x, y, col, w, out, st))

        def mha(eng=eng, x=x, y=y, sp=sp):
            host._chk(lib.ita_mha_long_f32(eng._h, 0, x.data_ptr(), y.data_ptr(), B, S, sp))

        def cols(eng=eng, x=x, st=st, sp=sp):
            host._chk(lib.ita_mha_long_f32_stats(eng._h, 0, x.data_ptr(), B, S, 1.0 / 256, C.byref(st), sp))

        def prop(R, eng=eng, x=x, w=w, out=out, sp=sp):
            wr = w[:, :R].contiguous()
            keep.append((wr,))
            return lambda: host._chk(lib.ita_mha_long_f32_propagate(eng._h, 0, x.data_ptr(), B, S, wr.data_ptr(), R, out.data_ptr(), sp))

        fns[f"mha_long_f32_E{E}"], fns[f"stats_cols_E{E}"] = mha, cols
        for R in ROWS:
            fns[f"propagate_R{R}_E{E}"] = prop(R)
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
        fig = dict(stats(v))
        if k.startswith("propagate_"):
            for name in ("mha_long_f32", "stats_cols"):
                base = t[f"{name}_E" + k.rsplit("_E", 1)[1]]
                fig["ratio_to_" + name] = {"of_medians": round(float(np.median(v)) / float(np.median(base)), 3),
                                           "lowest": round(min(v) / max(base), 3), "highest": round(max(v) / min(base), 3)}
        figures[k] = fig
    res = {"tool": "tools/bench_long_f32_propagate.py", "device": torch.cuda.get_device_name(0), "frames": B, "seq_len": S,
           "launches_per_round": a.launches, "rounds": a.rounds, "unit": "us per call",
           "mfma_count_ratio_to_mha_long_f32": {f"R{R}": round((2 * 192 + 16 * ((R + 15) // 16)) / (2 * 192), 3) for R in ROWS},
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
