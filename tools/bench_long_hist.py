#!/usr/bin/env python3
"""Cost of the long-sequence histograms (GPU box): 32 frames of S = 8192 tokens, E = 64 (vitlstm_E64_seed0: the FAST form)
and E = 128 (vit2l_E128_s0: the exact form), the blobs and inputs of tools/bench_long_stats.py.

  stats_all      ita_mha_long_int8_stats with all six outputs: the comparison call, on the same inputs in the same process
  hist_all       ita_mha_long_int8_hist with all five outputs: the projection launch + two Q K^T sweeps, three LDS atomic
                 adds per logit (logit bin, shift bin, and the row's shift class where the shift is below 8)
  hist_ls        the same with logits and shifts alone (no class counts)
  hist_probs     the same with probs alone (the class counts only: one add for the keys within 7 of the row maximum)
  ablate_all     with --ablate-so: hist_all of a build with -DITA_LONG_HIST_ABLATE=1, whose sweep 2 makes no histogram add
                 (its counts are wrong): hist_all minus this is what the counting costs

Device events around --launches calls after a warm-up, --rounds rounds with the figures interleaved; min / median / max
per figure and the ratio of the medians to stats_all of the same E.
usage: python tools/bench_long_hist.py [--out profiles/long_hist.json] [--ablate-so PATH] [--frames 32] [--seq 8192]
[--launches 10] [--rounds 5]"""
import argparse, ctypes as C, json, os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from drone_oa_iree_vit_accelerator_amd import host
from bench_long_layer import blob_of, stats, timed_us


def other_build(so, blob):
    """(library, handle) of another build of the library with the blob loaded, through its C ABI"""
    vp, ci = C.c_void_p, C.c_int
    L = C.CDLL(os.path.abspath(so))
    L.ita_create.argtypes = [C.POINTER(vp), ci]
    L.ita_destroy.argtypes = [vp]
    L.ita_load_weights.argtypes = [vp, vp, C.c_size_t]
    L.ita_error_string.restype = C.c_char_p
    L.ita_mha_long_int8_hist.argtypes = [vp, ci, vp, ci, ci, C.POINTER(host._MhaLongHist), vp]
    h = vp()
    for rc in (L.ita_create(C.byref(h), 0), L.ita_load_weights(h, C.create_string_buffer(blob, len(blob)), len(blob))):
        if rc:
            raise SystemExit(f"{so}: ita status {rc}: {L.ita_error_string().decode()}")
    return L, h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--ablate-so", default="")
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--seq", type=int, default=8192)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_long_hist.py measures on the GPU: none visible")
    B, S, lib = a.frames, a.seq, host.lib()
    fns, keep, others = {}, [], []
    for E in (128, 64):
        blob, s_x = blob_of(E)
        eng = host.Engine(blob, device=0)
        g = torch.Generator(device="cpu").manual_seed(5 + E)      # structured rows, as bench_long_stats.py builds them
        base = torch.randn((B, S // 32, E), generator=g).repeat_interleave(32, dim=1) * 18.0
        xq = (base + torch.randn((B, S, E), generator=g) * 9.0).round().clamp(-128, 127)
        x = ((xq + (torch.rand((B, S, E), generator=g) - 0.5) * 0.8) * s_x).cuda()
        sp = host._stream_ptr(0)
        so = {k: torch.empty((B, S), dtype=torch.int8 if k == "row_max" else torch.int32, device="cuda") for k in host.LONG_STATS}
        ho = {k: torch.empty((B, 2 if k in ("logits_out", "acc_range") else 256),
                             dtype=torch.int32 if k == "acc_range" else torch.int64, device="cuda") for k in host.LONG_HIST}
        st = host._MhaLongStats(**{k: v.data_ptr() for k, v in so.items()})
        keep.append((eng, x, so, ho, st))

        def stats_all(eng=eng, x=x, st=st, sp=sp):
            host._chk(lib.ita_mha_long_int8_stats(eng._h, 0, x.data_ptr(), B, S, C.byref(st), sp))

        def hist(names, L=lib, h=eng._h, x=x, ho=ho, sp=sp):
            s = host._MhaLongHist(**{k: ho[k].data_ptr() for k in names})
            keep.append((s,))

            def call():
                rc = L.ita_mha_long_int8_hist(h, 0, x.data_ptr(), B, S, C.byref(s), sp)
                if rc:
                    raise SystemExit(f"ita_mha_long_int8_hist: ita status {rc}")
            return call

        fns[f"stats_all_E{E}"] = stats_all
        fns[f"hist_all_E{E}"] = hist(host.LONG_HIST)
        fns[f"hist_ls_E{E}"] = hist(("logits", "shifts"))
        fns[f"hist_probs_E{E}"] = hist(("probs",))
        if a.ablate_so:
            L2, h2 = other_build(a.ablate_so, blob)
            others.append((L2, h2))
            fns[f"ablate_all_E{E}"] = hist(host.LONG_HIST, L=L2, h=h2)
    for f in fns.values():
        for _ in range(2):
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(a.rounds):
        for k, f in fns.items():       # interleaved: a drift of the box moves every figure alike
            t[k].append(timed_us(f, a.launches))
    res = {"tool": "tools/bench_long_hist.py", "device": torch.cuda.get_device_name(0), "frames": B, "seq_len": S,
           "launches_per_round": a.launches, "rounds": a.rounds, "unit": "us per call",
           "blobs": {"E64": "vitlstm_E64_seed0_B2 (one layer, FAST form)", "E128": "vit2l_E128_s0_B2 (two layers, exact form)"},
           "ablation_build": "-DITA_LONG_HIST_ABLATE=1: no LDS histogram adds in sweep 2" if a.ablate_so else None,
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
