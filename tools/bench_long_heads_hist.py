#!/usr/bin/env python3
"""Cost of the per-head long-sequence histograms (GPU box): ita_mha_long_heads_int8_hist at 32 frames of 8192 tokens, E = 64
(vitlstm_E64_seed0: the FAST requantisation form) and E = 128 (vit2l_E128_s0: the exact form), H = 2, 3, 4, 6, all five
outputs.

The weights do not depend on H, so one record per E is packed with each head count (tools/bench_long_heads.py).  Three
yardsticks in the same run: ita_mha_long_int8_hist on the H = 1 blob of the same weights (the design aims at a ratio below
H), ita_mha_long_heads_int8_stats (all six outputs) and ita_mha_long_heads_int8 on the same blob.

Device events around --launches calls after a warm-up, --rounds rounds with every figure of an E interleaved; min / median /
max and the rounds per figure.  usage: python tools/bench_long_heads_hist.py [--out profiles/long_heads_hist.json]
[--frames 32] [--seq 8192] [--launches 5] [--rounds 5]"""
import argparse, ctypes as C, json, os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from drone_oa_iree_vit_accelerator_amd import host, params
from bench_long_heads import HEADS, record_of, stats, timed_us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--seq", type=int, default=8192)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_long_heads_hist.py measures on the GPU: none visible")
    B, S, lib = a.frames, a.seq, host.lib()
    res = {"tool": "tools/bench_long_heads_hist.py", "device": torch.cuda.get_device_name(0), "frames": B, "seq_len": S,
           "launches_per_round": a.launches, "rounds": a.rounds, "unit": "us per call",
           "blobs": {"E64": "vitlstm_E64_seed0_B2 (FAST form)", "E128": "vit2l_E128_s0_B2 (exact form)"},
           "ratios": "over_H1_hist: median over ita_mha_long_int8_hist on the H = 1 blob; over_stats / over_mha: median over "
                     "ita_mha_long_heads_int8_stats (all six outputs) / ita_mha_long_heads_int8 on the same blob", "figures": {}}
    for E in (64, 128):
        d, fp, nl = record_of(E)
        s_x = 1.0 / float(params.attention_tensors(d, "attn0.", 0)["attn0.scal"][0])
        g = torch.Generator(device="cpu").manual_seed(5 + E)      # structured rows, as bench_long_heads.py builds them
        base = torch.randn((B, S // 32, E), generator=g).repeat_interleave(32, dim=1) * 18.0
        xq = (base + torch.randn((B, S, E), generator=g) * 9.0).round().clamp(-128, 127).cuda()
        x = ((xq + (torch.rand((B, S, E), generator=g).cuda() - 0.5) * 0.8) * s_x).contiguous()
        y, sp = torch.empty_like(x), host._stream_ptr(0)
        engs, fns = [], {}
        for H in HEADS:
            eng = host.Engine(params.blob_from_record(d, fp, E=E, num_layers=nl, H=H), device=0)
            engs.append(eng)
            width = dict(logits=256, logits_out=2, acc_range=2, shifts=256, probs=256)
            ho = {k: torch.empty((B, H, width[k]), dtype=torch.int32 if k == "acc_range" else torch.int64, device="cuda") for k in host.LONG_HIST}
            hs = host._MhaLongHist(**{k: v.data_ptr() for k, v in ho.items()})
            if H == 1:
                def one(eng=eng, hs=hs, ho=ho):
                    host._chk(lib.ita_mha_long_int8_hist(eng._h, 0, x.data_ptr(), B, S, C.byref(hs), sp))
                fns[(1, "hist")] = one
                continue
            so = {k: torch.empty((B, H, S), dtype=torch.int8 if k == "row_max" else torch.int32, device="cuda") for k in host.LONG_STATS}
            ss = host._MhaLongStats(**{k: v.data_ptr() for k, v in so.items()})

            def hist(eng=eng, hs=hs, ho=ho):
                host._chk(lib.ita_mha_long_heads_int8_hist(eng._h, 0, x.data_ptr(), B, S, C.byref(hs), sp))

            def sts(eng=eng, ss=ss, so=so):
                host._chk(lib.ita_mha_long_heads_int8_stats(eng._h, 0, x.data_ptr(), B, S, C.byref(ss), sp))

            def mha(eng=eng):
                host._chk(lib.ita_mha_long_heads_int8(eng._h, 0, x.data_ptr(), y.data_ptr(), B, S, sp))
            fns[(H, "hist")], fns[(H, "stats")], fns[(H, "mha")] = hist, sts, mha
        for f in fns.values():
            for _ in range(2):
                f()
        torch.cuda.synchronize()
        t = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, f in fns.items():      # interleaved: a drift of the box moves every figure alike
                t[k].append(timed_us(f, a.launches))
        med = {k: float(np.median(v)) for k, v in t.items()}
        for (H, form), v in t.items():
            fig = stats(v)
            if form == "hist" and H > 1:
                fig.update(over_H1_hist=round(med[(H, form)] / med[(1, "hist")], 3), over_stats=round(med[(H, form)] / med[(H, "stats")], 3),
                           over_mha=round(med[(H, form)] / med[(H, "mha")], 3))
            res["figures"][f"E{E}_H{H}_{form}"] = fig
        for eng in engs:
            eng.close()
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
