#!/usr/bin/env python3
"""Cost of attention heads on long sequences (GPU box): ita_mha_long_heads_int8 at 32 frames of 8192 tokens, E = 64
(vitlstm_E64_seed0: the FAST requantisation form) and E = 128 (vit2l_E128_s0: the exact form), H = 2, 3, 4, 6.

The weights do not depend on H, so one record per E is packed with each head count; the yardstick is ita_mha_long_int8 on
the H = 1 blob of the same weights (only the header's H differs).  The projection launch is the same in every call, so
the ratio prices ita_long_heads_attn_kernel<.., H, ..> against ita_long_attn_kernel.

Device events around --launches calls after a warm-up, --rounds rounds with the head counts interleaved; min / median /
max per figure.  usage: python tools/bench_long_heads.py [--out profiles/long_heads.json] [--frames 32] [--seq 8192]
[--launches 5] [--rounds 5]"""
import argparse, json, os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from drone_oa_iree_vit_accelerator_amd import host, params, synth

HEADS = (1, 2, 3, 4, 6)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")


def record_of(E):
    if E == 64:
        return params.load_fixture(os.path.join(GOLDEN, "vitlstm_E64_seed0_B2.npz")), synth.float_params(0, E=64), 1
    return params.load_fixture(os.path.join(GOLDEN, "vit2l_E128_s0_B2.npz")), synth.float_params(0, E=128, num_layers=2, tail=False), 2


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
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_long_heads.py measures on the GPU: none visible")
    B, S, lib = a.frames, a.seq, host.lib()
    res = {"tool": "tools/bench_long_heads.py", "device": torch.cuda.get_device_name(0), "frames": B, "seq_len": S,
           "launches_per_round": a.launches, "rounds": a.rounds, "unit": "us per call",
           "blobs": {"E64": "vitlstm_E64_seed0_B2 (FAST form)", "E128": "vit2l_E128_s0_B2 (exact form)"}, "figures": {}}
    for E in (64, 128):
        d, fp, nl = record_of(E)
        s_x = 1.0 / float(params.attention_tensors(d, "attn0.", 0)["attn0.scal"][0])
        g = torch.Generator(device="cpu").manual_seed(5 + E)      # structured rows, as bench_long_layer.py builds them
        base = torch.randn((B, S // 32, E), generator=g).repeat_interleave(32, dim=1) * 18.0
        xq = (base + torch.randn((B, S, E), generator=g) * 9.0).round().clamp(-128, 127).cuda()
        x = ((xq + (torch.rand((B, S, E), generator=g).cuda() - 0.5) * 0.8) * s_x).contiguous()
        y, sp = torch.empty_like(x), host._stream_ptr(0)
        engs, fns = [], {}
        for H in HEADS:
            eng = host.Engine(params.blob_from_record(d, fp, E=E, num_layers=nl, H=H), device=0)
            engs.append(eng)
            entry = lib.ita_mha_long_int8 if H == 1 else lib.ita_mha_long_heads_int8

            def call(eng=eng, entry=entry):
                host._chk(entry(eng._h, 0, x.data_ptr(), y.data_ptr(), B, S, sp))
            fns[H] = call
        for f in fns.values():
            for _ in range(2):
                f()
        torch.cuda.synchronize()
        t = {H: [] for H in HEADS}
        for _ in range(a.rounds):
            for H in HEADS:            # interleaved: a drift of the box moves every head count alike
                t[H].append(timed_us(fns[H], a.launches))
        one = float(np.median(t[1]))
        for H in HEADS:
            res["figures"][f"E{E}_H{H}"] = {**stats(t[H]), "over_H1": round(float(np.median(t[H])) / one, 3),
                                            "frames_per_s": round(B / float(np.median(t[H])) * 1e6, 1)}
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
