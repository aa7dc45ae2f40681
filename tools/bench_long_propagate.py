#!/usr/bin/env python3
"""Cost of the long-sequence propagation (GPU box): 32 frames of S = 8192 tokens, E = 64 (vitlstm_E64_seed0: the FAST
form) and E = 128 (vit2l_E128_s0: the exact form), the blobs and inputs of tools/bench_long_layer.py.

  mha_long       ita_mha_long_int8 of this build: projection launch + three Q K^T sweeps + A.V + out_proj
  stats_all      ita_mha_long_int8_stats with all six outputs: projection + three sweeps, reduced along rows and columns
  stats_rowmax   ita_mha_long_int8_stats with row_max and row_sum alone: what the propagation runs as its second launch
  propagate_nN   ita_mha_long_int8_propagate with n_w = N weight rows (1, 16, 64): projection + the statistics launch +
                 the prep launch + the transposed sweep (one more Q K^T sweep and 2 ceil(N / 16) MFMAs per lane and tile)

Device events around --launches calls after a warm-up, --rounds rounds with the figures interleaved in one process on the
same inputs; min / median / max per figure and the ratio of the medians to mha_long and to stats_all.
usage: python tools/bench_long_propagate.py [--out profiles/long_propagate.json] [--frames 32] [--seq 8192]
[--launches 10] [--rounds 5]"""
import argparse, ctypes as C, json, os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from drone_oa_iree_vit_accelerator_amd import host
from bench_long_layer import blob_of, stats, timed_us

N_W = (1, 16, 64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--seq", type=int, default=8192)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_long_propagate.py measures on the GPU: none visible")
    B, S, lib = a.frames, a.seq, host.lib()
    fns, written, keep = {}, {}, []
    for E in (128, 64):
        blob, s_x = blob_of(E)
        eng = host.Engine(blob, device=0)
        g = torch.Generator(device="cpu").manual_seed(5 + E)      # structured rows, as bench_long_layer.py builds them
        base = torch.randn((B, S // 32, E), generator=g).repeat_interleave(32, dim=1) * 18.0
        xq = (base + torch.randn((B, S, E), generator=g) * 9.0).round().clamp(-128, 127)
        x = ((xq + (torch.rand((B, S, E), generator=g) - 0.5) * 0.8) * s_x).cuda()
        y, sp = torch.empty_like(x), host._stream_ptr(0)
        st_out = {k: torch.empty((B, S), dtype=torch.int8 if k == "row_max" else torch.int32, device="cuda") for k in host.LONG_STATS}
        w = torch.randint(-127, 128, (B, max(N_W), S), generator=g, dtype=torch.int8).cuda()
        out = torch.empty((B, max(N_W), S), dtype=torch.int32, device="cuda")
        keep.append((eng, x, y, st_out, w, out))

        def mha(eng=eng, x=x, y=y, sp=sp):
            host._chk(lib.ita_mha_long_int8(eng._h, 0, x.data_ptr(), y.data_ptr(), B, S, sp))

        def st(names, eng=eng, x=x, st_out=st_out, sp=sp):
            s = host._MhaLongStats(**{k: st_out[k].data_ptr() for k in names})
            keep.append((s,))
            return lambda: host._chk(lib.ita_mha_long_int8_stats(eng._h, 0, x.data_ptr(), B, S, C.byref(s), sp))

        def prop(n, eng=eng, x=x, w=w, out=out, sp=sp):
            wn = w[:, :n].contiguous()
            keep.append((wn,))
            return lambda: host._chk(lib.ita_mha_long_int8_propagate(eng._h, 0, x.data_ptr(), B, S, wn.data_ptr(), n,
                                                                     out.data_ptr(), sp))

        for key, f, nbytes in [(f"mha_long_E{E}", mha, B * S * E * 4), (f"stats_all_E{E}", st(host.LONG_STATS), B * S * 21),
                               (f"stats_rowmax_E{E}", st(("row_max", "row_sum")), B * S * 5)] + \
                              [(f"propagate_n{n}_E{E}", prop(n), B * n * S * 4) for n in N_W]:
            fns[key], written[key] = f, nbytes
    for f in fns.values():
        for _ in range(2):
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(a.rounds):
        for k, f in fns.items():       # interleaved: a drift of the box moves every figure alike
            t[k].append(timed_us(f, a.launches))
    med = lambda k: float(np.median(t[k]))
    res = {"tool": "tools/bench_long_propagate.py", "device": torch.cuda.get_device_name(0), "frames": B, "seq_len": S,
           "launches_per_round": a.launches, "rounds": a.rounds, "unit": "us per call",
           "blobs": {"E64": "vitlstm_E64_seed0_B2 (one layer, FAST form)", "E128": "vit2l_E128_s0_B2 (two layers, exact form)"},
           "figures": {k: {**stats(v), "bytes_written": written[k],
                           "ratio_to_mha_long": round(med(k) / med("mha_long_E" + k.rsplit("_E", 1)[1]), 3),
                           "ratio_to_stats_all": round(med(k) / med("stats_all_E" + k.rsplit("_E", 1)[1]), 3)}
                       for k, v in t.items()}}
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
