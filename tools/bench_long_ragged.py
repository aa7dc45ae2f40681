#!/usr/bin/env python3
"""Cost of ragged batches on long sequences (GPU box): ita_mha_long_int8_ragged at E = 128 (vit2l_E128_s0), 32 frames with
a stride of 8192 tokens, against ita_mha_long_int8 (whose kernels this feature leaves as they were):
    (a) full      every length 8192             / ita_mha_long_int8 at 8192: the price of the length read and the tail branch
    (b) len4097   every length 4097             / ita_mha_long_int8 at 4224   } the nearest multiples of 128 a caller could
        len1200   every length 1200             / ita_mha_long_int8 at 1280   } pad to if masking did not matter
    (c) mixed     lengths spread over 128..8192 / ita_mha_long_int8 at 8192: the saving from work that follows len squared
The ragged calls keep the stride 8192 throughout: their projection launch covers every padded tile.

Device events around --launches calls after a warm-up, --rounds rounds with all figures interleaved; min / median / max.
usage: python tools/bench_long_ragged.py [--out profiles/long_ragged.json] [--frames 32] [--seq 8192] [--launches 40] [--rounds 7]"""
import argparse, json, os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from drone_oa_iree_vit_accelerator_amd import host
from bench_long_layer import blob_of, stats, timed_us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--seq", type=int, default=8192)
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_long_ragged.py measures on the GPU: none visible")
    B, S, E, lib = a.frames, a.seq, 128, host.lib()
    blob, s_x = blob_of(E)
    eng = host.Engine(blob, device=0)
    g = torch.Generator(device="cpu").manual_seed(5 + E)      # structured rows, as bench_long_layer.py builds them
    base = torch.randn((B, S // 32, E), generator=g).repeat_interleave(32, dim=1) * 18.0
    xq = (base + torch.randn((B, S, E), generator=g) * 9.0).round().clamp(-128, 127).cuda()
    x = ((xq + (torch.rand((B, S, E), generator=g).cuda() - 0.5) * 0.8) * s_x).contiguous()
    y, sp = torch.empty_like(x), host._stream_ptr(0)
    up = lambda n: (n + 127) // 128 * 128
    mixed = [int(v) for v in np.linspace(128, S, B).round()]
    lens = {"full": [S] * B, "len4097": [4097 * S // 8192] * B, "len1200": [1200 * S // 8192] * B, "mixed": mixed}
    against = {"full": S, "len4097": up(lens["len4097"][0]), "len1200": up(lens["len1200"][0]), "mixed": S}
    dev = {k: torch.tensor(v, dtype=torch.int32, device="cuda") for k, v in lens.items()}
    xs = {s: x[:, :s].contiguous() for s in set(against.values())}      # what a caller who pads to a multiple of 128 hands over
    fns = {}
    for k in lens:
        fns[k] = lambda k=k: host._chk(lib.ita_mha_long_int8_ragged(eng._h, 0, x.data_ptr(), y.data_ptr(), B, S, dev[k].data_ptr(), sp))
    for s, v in xs.items():
        fns[f"long_{s}"] = lambda s=s, v=v: host._chk(lib.ita_mha_long_int8(eng._h, 0, v.data_ptr(), y.data_ptr(), B, s, sp))
    fns["long_%d" % S]()                                                # the workspace at its largest before anything is timed
    full = y.clone()
    fns["full"]()
    same = bool(torch.equal(y, full))
    for f in fns.values():
        for _ in range(2):
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(a.rounds):
        for k, f in fns.items():            # interleaved: a drift of the box moves every figure alike
            t[k].append(timed_us(f, a.launches))
    res = {"tool": "tools/bench_long_ragged.py", "device": torch.cuda.get_device_name(0), "E": E, "frames": B, "seq_stride": S,
           "launches_per_round": a.launches, "rounds": a.rounds, "unit": "us per call (projection + attention launch)",
           "blob": "vit2l_E128_s0_B2 (exact form)", "full_lengths_equal_mha_long_bits": same, "mixed_lens": mixed, "figures": {}}
    for k, v in t.items():
        res["figures"][k] = stats(v)
    for k in lens:
        ref = f"long_{against[k]}"
        res["figures"][k].update(lens=lens[k][0] if k != "mixed" else "mixed_lens", against=ref,
                                 over_against=round(float(np.median(t[k])) / float(np.median(t[ref])), 3))
    eng.close()
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
