#!/usr/bin/env python3
"""Cost of the per-head weighted column sums on long sequences (GPU box): ita_mha_long_heads_int8_propagate at 32 frames of
8192 tokens, n_w = 16 and 64 weight rows, E = 64 (vitlstm_E64_seed0: the FAST requantisation form) and E = 128
(vit2l_E128_s0: the exact form), H = 2, 3, 4, 6.

The weights do not depend on H, so one record per E is packed with each head count (tools/bench_long_heads.py).  Two
yardsticks, measured in the same run: ita_mha_long_int8_propagate on the H = 1 blob of the same weights with the same n_w
(H one-head calls would give the H outputs of one heads call if the heads were separate blobs: the design's claim is
over_H1 < H, since the projection, the staging and the launches are shared), and ita_mha_long_heads_int8 on the same blob
(the attention whose probabilities are summed).

Device events around --launches calls after a warm-up, --rounds rounds with every figure of an E interleaved; min / median /
max and the rounds per figure.  usage: python tools/bench_long_heads_propagate.py [--out profiles/long_heads_propagate.json]
[--frames 32] [--seq 8192] [--launches 5] [--rounds 5]"""
import argparse, json, os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from drone_oa_iree_vit_accelerator_amd import host, params
from bench_long_heads import HEADS, record_of, stats, timed_us

ROWS = (16, 64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--seq", type=int, default=8192)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_long_heads_propagate.py measures on the GPU: none visible")
    B, S, lib = a.frames, a.seq, host.lib()
    res = {"tool": "tools/bench_long_heads_propagate.py", "device": torch.cuda.get_device_name(0), "frames": B, "seq_len": S,
           "launches_per_round": a.launches, "rounds": a.rounds, "unit": "us per call",
           "blobs": {"E64": "vitlstm_E64_seed0_B2 (FAST form)", "E128": "vit2l_E128_s0_B2 (exact form)"},
           "ratios": "over_H1: median over ita_mha_long_int8_propagate on the H = 1 blob at the same n_w (the claim: below H); "
                     "over_mha: median over ita_mha_long_heads_int8 on the same blob", "figures": {}}
    for E in (64, 128):
        d, fp, nl = record_of(E)
        s_x = 1.0 / float(params.attention_tensors(d, "attn0.", 0)["attn0.scal"][0])
        g = torch.Generator(device="cpu").manual_seed(5 + E)      # structured rows, as bench_long_heads.py builds them
        base = torch.randn((B, S // 32, E), generator=g).repeat_interleave(32, dim=1) * 18.0
        xq = (base + torch.randn((B, S, E), generator=g) * 9.0).round().clamp(-128, 127).cuda()
        x = ((xq + (torch.rand((B, S, E), generator=g).cuda() - 0.5) * 0.8) * s_x).contiguous()
        w = torch.randint(-127, 128, (B, max(ROWS), S), generator=g, dtype=torch.int8).cuda()
        y, sp = torch.empty_like(x), host._stream_ptr(0)
        out = torch.empty((B, max(HEADS), max(ROWS), S), dtype=torch.int32, device="cuda")      # every call's output fits
        engs, fns = [], {}
        for H in HEADS:
            eng = host.Engine(params.blob_from_record(d, fp, E=E, num_layers=nl, H=H), device=0)
            engs.append(eng)
            if H > 1:
                def mha(eng=eng):
                    host._chk(lib.ita_mha_long_heads_int8(eng._h, 0, x.data_ptr(), y.data_ptr(), B, S, sp))
                fns[(H, "mha")] = mha
            entry = lib.ita_mha_long_int8_propagate if H == 1 else lib.ita_mha_long_heads_int8_propagate
            for R in ROWS:
                wr = w[:, :R].contiguous()

                def call(eng=eng, entry=entry, wr=wr, R=R):
                    host._chk(entry(eng._h, 0, x.data_ptr(), B, S, wr.data_ptr(), R, out.data_ptr(), sp))
                fns[(H, R)] = call
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
            if form != "mha":
                fig["over_H1"] = round(med[(H, form)] / med[(1, form)], 3)
            if H > 1:
                fig["over_mha"] = round(med[(H, form)] / med[(H, "mha")], 3)
            res["figures"][f"E{E}_H{H}_" + (form if form == "mha" else f"nw{form}")] = fig
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
