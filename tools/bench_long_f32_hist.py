#!/usr/bin/env python3
"""Cost of the long float histograms (GPU box): 32 frames of S = 8192 tokens, the ITAW0003 blobs and inputs of
tools/bench_long_f32.py at E = 64 and E = 128, every figure on the same blob and handle.

  mha_long_f32   ita_mha_long_f32: projection launch + one sweep of Q K^T, running softmax and P V + out_proj
  stats_all      ita_mha_long_f32_stats with all six outputs: the comparison call, the same two sweeps of Q K^T
  hist_all       ita_mha_long_f32_hist with all five outputs: the zeroing kernel, the projection launch, two sweeps, three
                 wave-aggregated LDS adds per element
  hist_range     the same with range alone: one sweep
  ablate_all     with --ablate-so: hist_all of a build with -DITA_LF32_HIST_ABLATE=1, which forms every bin and makes no LDS
                 add (its counts are wrong): hist_all minus this is what the counting costs
  plain_all      with --plain-so: hist_all of a build with -DITA_LF32_HIST_ABLATE=2, one add per lane without the
                 aggregation inside the wave (its counts are right): this minus hist_all is what the aggregation saves
  *_flat         the same calls on x = 0: every query and every key is its bias, all logits are equal and each histogram has one
                 hot bin (the flat-row case)

Device events around --launches calls after a warm-up, --rounds rounds with the figures interleaved so that a drift of the
box moves every figure alike; min / median / max per figure and the ratio of the medians to stats_all of the same E.
usage: python tools/bench_long_f32_hist.py [--out profiles/long_f32_hist.json] [--ablate-so PATH] [--plain-so PATH]
[--frames 32] [--seq 8192] [--launches 3] [--rounds 7] [--scale 1.0]"""
import argparse, ctypes as C, json, os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from drone_oa_iree_vit_accelerator_amd import host, params, synth
from bench_long_f32 import LAYERS, stats, timed_us


def other_build(so, blob):
    """(library, handle) of another build of the library with the blob loaded, through its C ABI"""
    vp, ci = C.c_void_p, C.c_int
    L = C.CDLL(os.path.abspath(so))
    L.ita_create.argtypes = [C.POINTER(vp), ci]
    L.ita_destroy.argtypes = [vp]
    L.ita_load_weights.argtypes = [vp, vp, C.c_size_t]
    L.ita_error_string.restype = C.c_char_p
    L.ita_mha_long_f32_hist.argtypes = [vp, ci, vp, ci, ci, C.c_float, C.POINTER(host._MhaLongF32Hist), vp]
    h = vp()
    for rc in (L.ita_create(C.byref(h), 0), L.ita_load_weights(h, C.create_string_buffer(blob, len(blob)), len(blob))):
        if rc:
            raise SystemExit(f"{so}: ita status {rc}: {L.ita_error_string().decode()}")
    return L, h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--ablate-so", default="")
    ap.add_argument("--plain-so", default="")
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--seq", type=int, default=8192)
    ap.add_argument("--launches", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--scale", type=float, default=1.0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_long_f32_hist.py measures on the GPU: none visible")
    B, S, lib = a.frames, a.seq, host.lib()
    fns, keep, others = {}, [], []
    for E in (128, 64):
        L = LAYERS[E]
        blob = params.blob_from_float_params(synth.float_params(E, E=E, num_layers=L, tail=(E == 64)), L)
        eng = host.Engine(blob, device=0)
        g = torch.Generator(device="cpu").manual_seed(5 + E)      # LayerNorm-like rows, as bench_long_f32.py builds them
        x = torch.randn((B, S, E), generator=g)
        x = ((x - x.mean(-1, keepdim=True)) / x.std(-1, keepdim=True, unbiased=False)).cuda()
        x0 = torch.zeros_like(x)
        y, sp = torch.empty_like(x), host._stream_ptr(0)
        so = {k: torch.empty((B, S), dtype=torch.int32 if k.endswith("_nnz") else torch.float32, device="cuda")
              for k in host.LONG_F32_STATS}
        ho = {k: torch.empty((B, 2 if k in ("logits_out", "range") else 256),
                             dtype=torch.float32 if k == "range" else torch.int64, device="cuda") for k in host.LONG_F32_HIST}
        st = host._MhaLongF32Stats(**{k: v.data_ptr() for k, v in so.items()})
        keep.append((eng, x, x0, y, so, ho, st))

        def mha(eng=eng, x=x, y=y, sp=sp):
            host._chk(lib.ita_mha_long_f32(eng._h, 0, x.data_ptr(), y.data_ptr(), B, S, sp))

        def stats_all(eng=eng, x=x, st=st, sp=sp):
            host._chk(lib.ita_mha_long_f32_stats(eng._h, 0, x.data_ptr(), B, S, 1.0 / 256, C.byref(st), sp))

        def hist(names, x=x, L=lib, h=eng._h, ho=ho, sp=sp):
            s = host._MhaLongF32Hist(**{k: ho[k].data_ptr() for k in names})
            keep.append((s,))

            def call():
                rc = L.ita_mha_long_f32_hist(h, 0, x.data_ptr(), B, S, a.scale, C.byref(s), sp)
                if rc:
                    raise SystemExit(f"ita_mha_long_f32_hist: ita status {rc}")
            return call

        fns[f"mha_long_f32_E{E}"] = mha
        fns[f"stats_all_E{E}"] = stats_all
        fns[f"hist_all_E{E}"] = hist(host.LONG_F32_HIST)
        fns[f"hist_range_E{E}"] = hist(("range",))
        fns[f"hist_all_flat_E{E}"] = hist(host.LONG_F32_HIST, x=x0)
        for key, path in (("ablate", a.ablate_so), ("plain", a.plain_so)):
            if path:
                L2, h2 = other_build(path, blob)
                others.append((L2, h2))
                fns[f"{key}_all_E{E}"] = hist(host.LONG_F32_HIST, L=L2, h=h2)
                fns[f"{key}_all_flat_E{E}"] = hist(host.LONG_F32_HIST, x=x0, L=L2, h=h2)
    for f in fns.values():
        for _ in range(2):
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(a.rounds):
        for k, f in fns.items():       # interleaved: a drift of the box moves every figure alike
            t[k].append(timed_us(f, a.launches))
    res = {"tool": "tools/bench_long_f32_hist.py", "device": torch.cuda.get_device_name(0), "frames": B, "seq_len": S,
           "launches_per_round": a.launches, "rounds": a.rounds, "unit": "us per call", "scale": a.scale,
           "blobs": {"E64": "synth.float_params(64, E=64), one layer, ITAW0003", "E128": "synth.float_params(128, E=128, num_layers=2, tail=False), ITAW0003"},
           "inputs": {"default": "LayerNorm-like rows (hot bins: shifts 255, probs 0 .. 2)", "_flat": "x = 0: every logit equal, one hot bin per histogram"},
           "ablation_builds": {"ablate": "-DITA_LF32_HIST_ABLATE=1: bins formed, no LDS add" if a.ablate_so else None,
                               "plain": "-DITA_LF32_HIST_ABLATE=2: one LDS add per lane, no aggregation" if a.plain_so else None},
           "figures": {k: {**stats(v),
                           "ratio_to_stats_all": round(float(np.median(v)) / float(np.median(t["stats_all_E" + k.rsplit("_E", 1)[1]])), 3)}
                       for k, v in t.items()}}
    for L2, h2 in others:
        L2.ita_destroy(h2)
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
