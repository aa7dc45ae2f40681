#!/usr/bin/env python3
"""Cost of ragged batches on the long FLOAT path (GPU box): ita_mha_long_f32_ragged at E = 128 (ITAW0003, two layers, layer
0), 32 frames with a stride of 8192 tokens -- the float workspace is 192 KB per 128-token tile, 384 MB here, the shape
tools/bench_long_f32.py measures -- against ita_mha_long_f32 of the same library (whose kernels this feature leaves as
they were):
    (a) full      every length 8192             / ita_mha_long_f32 at 8192: the price of the length reads and the tail branch,
                  reported beside the min .. max spread of the parent's own rounds (inside_parent_spread)
    (b) len4097   every length 4097             / ita_mha_long_f32 at 4224   } the nearest multiples of 128 a caller could
        len1200   every length 1200             / ita_mha_long_f32 at 1280   } pad to if masking did not matter
    (c) mixed     lengths spread over 128..8192 / ita_mha_long_f32 at 8192, beside mean(len^2) / stride^2: the attention
                  sweep's work follows len squared
The ragged calls keep the stride 8192 throughout; their projection launch skips the 64-key units past a frame's length.

Device events around --launches calls after a warm-up, --rounds rounds with all figures interleaved; min / median / max.
usage: python tools/bench_long_ragged_f32.py [--out profiles/long_ragged_f32.json] [--frames 32] [--seq 8192] [--launches 5] [--rounds 7]"""
import argparse, json, os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from drone_oa_iree_vit_accelerator_amd import host, params, synth
from bench_long_layer import stats, timed_us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--seq", type=int, default=8192)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_long_ragged_f32.py measures on the GPU: none visible")
    B, S, E, lib = a.frames, a.seq, 128, host.lib()
    eng = host.Engine(params.blob_from_float_params(synth.float_params(E, E=E, num_layers=2, tail=False), 2), device=0)
    g = torch.Generator(device="cpu").manual_seed(5 + E)      # LayerNorm-like rows, as bench_long_f32.py builds them
    x = torch.randn((B, S, E), generator=g)
    x = ((x - x.mean(-1, keepdim=True)) / x.std(-1, keepdim=True, unbiased=False)).cuda().contiguous()
    y, sp = torch.empty_like(x), host._stream_ptr(0)
    up = lambda n: (n + 127) // 128 * 128
    mixed = [int(v) for v in np.linspace(128, S, B).round()]
    lens = {"full": [S] * B, "len4097": [4097 * S // 8192] * B, "len1200": [1200 * S // 8192] * B, "mixed": mixed}
    against = {"full": S, "len4097": up(lens["len4097"][0]), "len1200": up(lens["len1200"][0]), "mixed": S}
    dev = {k: torch.tensor(v, dtype=torch.int32, device="cuda") for k, v in lens.items()}
    xs = {s: x[:, :s].contiguous() for s in set(against.values())}      # what a caller who pads to a multiple of 128 hands over
    fns = {}
    for k in lens:
        fns[k] = lambda k=k: host._chk(lib.ita_mha_long_f32_ragged(eng._h, 0, x.data_ptr(), y.data_ptr(), B, S, dev[k].data_ptr(), sp))
    for s, v in xs.items():
        fns[f"long_{s}"] = lambda s=s, v=v: host._chk(lib.ita_mha_long_f32(eng._h, 0, v.data_ptr(), y.data_ptr(), B, s, sp))
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
    res = {"tool": "tools/bench_long_ragged_f32.py", "device": torch.cuda.get_device_name(0), "E": E, "frames": B, "seq_stride": S,
           "launches_per_round": a.launches, "rounds": a.rounds, "unit": "us per call (projection + attention launch)",
           "blob": "synth.float_params(128, E=128, num_layers=2, tail=False), ITAW0003, layer 0",
           "workspace_bytes": B * (S // 128) * 4 * 49152, "full_lengths_equal_mha_long_f32_bits": same, "mixed_lens": mixed,
           "mixed_mean_len2_over_stride2": round(float(np.mean(np.square(np.array(mixed, np.float64) / S))), 3), "figures": {}}
    for k, v in t.items():
        res["figures"][k] = stats(v)
    for k in lens:
        ref = f"long_{against[k]}"
        res["figures"][k].update(lens=lens[k][0] if k != "mixed" else "mixed_lens", against=ref,
                                 over_against=round(float(np.median(t[k])) / float(np.median(t[ref])), 3))
    parent = t[f"long_{S}"]
    res["figures"]["full"]["inside_parent_spread"] = bool(min(parent) <= float(np.median(t["full"])) <= max(parent))
    eng.close()
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
