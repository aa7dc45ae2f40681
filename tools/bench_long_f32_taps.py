#!/usr/bin/env python3
"""Cost of the long float taps (GPU box): 32 frames of S = 8192 tokens, the ITAW0003 blobs and inputs of
tools/bench_long_f32.py at E = 64 and E = 128.

  mha_long_f32          ita_mha_long_f32 of this build (the production kernels)
  mha_long_f32_parent   the same entry of another build of the library (--parent-so: the commit before the taps), loaded
                        beside this one in the same process and timed in the same rounds
  taps_null             ita_mha_long_f32_taps with every tap NULL: the taps kernels, no extra store
  taps_probs16          the same with probs for 16 query rows (the logits go to the probs buffer, the handle keeps
                        row_max and row_sum, and the elementwise launch turns them into probabilities in place)
  taps_all              the four stage tensors (Q, K, V, ctx) and logits, probs, row_max, row_sum of 16 rows

Device events around --launches calls after a warm-up, --rounds rounds with the figures interleaved; min / median / max
per figure, and the bytes each variant writes (y and the taps; the workspace traffic is the same for all).  Recorded, not
gated.  usage: python tools/bench_long_f32_taps.py [--out profiles/long_f32_taps.json] [--parent-so PATH] [--frames 32]
[--seq 8192] [--launches 3] [--rounds 5]"""
import argparse, ctypes as C, json, os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from drone_oa_iree_vit_accelerator_amd import host, params, synth
from bench_long_f32 import LAYERS, stats, timed_us


class OtherBuild:
    """ita_mha_long_f32 of another build of the library: its own handle and weights"""

    def __init__(self, so, blob):
        self.lib = C.CDLL(os.path.abspath(so))
        vp, i = C.c_void_p, C.c_int
        self.lib.ita_create.argtypes = [C.POINTER(vp), i]
        self.lib.ita_destroy.argtypes = [vp]
        self.lib.ita_load_weights.argtypes = [vp, vp, C.c_size_t]
        self.lib.ita_mha_long_f32.argtypes = [vp, i, vp, vp, i, i, vp]
        self.lib.ita_error_string.restype = C.c_char_p
        self.h = vp()
        self.chk(self.lib.ita_create(C.byref(self.h), 0))
        buf = C.create_string_buffer(blob, len(blob))
        self.chk(self.lib.ita_load_weights(self.h, buf, len(blob)))

    def chk(self, rc):
        if rc:
            raise SystemExit(f"--parent-so: ita status {rc}: {self.lib.ita_error_string().decode()}")

    def close(self):
        self.lib.ita_destroy(self.h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--parent-so", default="")
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--seq", type=int, default=8192)
    ap.add_argument("--launches", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_long_f32_taps.py measures on the GPU: none visible")
    B, S, lib, P = a.frames, a.seq, host.lib(), 192
    fns, nbytes, keep = {}, {}, []
    for E in (128, 64):
        L = LAYERS[E]
        blob = params.blob_from_float_params(synth.float_params(E, E=E, num_layers=L, tail=(E == 64)), L)
        eng = host.Engine(blob, device=0)
        g = torch.Generator(device="cpu").manual_seed(5 + E)      # LayerNorm-like rows, as bench_long_f32.py builds them
        x = torch.randn((B, S, E), generator=g)
        x = ((x - x.mean(-1, keepdim=True)) / x.std(-1, keepdim=True, unbiased=False)).cuda()
        y, sp = torch.empty_like(x), host._stream_ptr(0)
        rows = list(range(0, S, S // 16))[:16]
        arr = (C.c_int * 16)(*rows)
        mk = lambda *s: torch.empty(s, dtype=torch.float32, device="cuda")
        rowt = dict(logits=mk(B, 16, S), probs=mk(B, 16, S), row_max=mk(B, 16), row_sum=mk(B, 16))
        tens = dict(Q=mk(B, S, P), K=mk(B, S, P), V=mk(B, S, P), ctx=mk(B, S, P))
        st_null = host._MhaLongF32Taps()
        st_probs = host._MhaLongF32Taps(probs=rowt["probs"].data_ptr())
        st_probs.rows, st_probs.n_rows = arr, 16
        st_all = host._MhaLongF32Taps(**{k: v.data_ptr() for k, v in {**tens, **rowt}.items()})
        st_all.rows, st_all.n_rows = arr, 16
        keep.append((eng, x, y, arr, rowt, tens))

        def mha(eng=eng, x=x, y=y, sp=sp):
            host._chk(lib.ita_mha_long_f32(eng._h, 0, x.data_ptr(), y.data_ptr(), B, S, sp))

        def taps(st, eng=eng, x=x, y=y, sp=sp):
            return lambda: host._chk(lib.ita_mha_long_f32_taps(eng._h, 0, x.data_ptr(), y.data_ptr(), B, S, C.byref(st), sp))

        ybytes, rowbytes = B * S * E * 4, B * 16 * S * 4
        fns[f"mha_long_f32_E{E}"], nbytes[f"mha_long_f32_E{E}"] = mha, ybytes
        if a.parent_so:
            other = OtherBuild(a.parent_so, blob)
            keep.append((other,))

            def parent(other=other, x=x, y=y, sp=sp):
                other.chk(other.lib.ita_mha_long_f32(other.h, 0, x.data_ptr(), y.data_ptr(), B, S, sp))
            fns[f"mha_long_f32_parent_E{E}"], nbytes[f"mha_long_f32_parent_E{E}"] = parent, ybytes
        fns[f"taps_null_E{E}"], nbytes[f"taps_null_E{E}"] = taps(st_null), ybytes
        fns[f"taps_probs16_E{E}"], nbytes[f"taps_probs16_E{E}"] = taps(st_probs), ybytes + 2 * rowbytes + 2 * B * 16 * 4
        fns[f"taps_all_E{E}"], nbytes[f"taps_all_E{E}"] = taps(st_all), ybytes + 4 * B * S * P * 4 + 2 * rowbytes + 2 * B * 16 * 4
    for f in fns.values():
        for _ in range(2):
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(a.rounds):
        for k, f in fns.items():       # interleaved: a drift of the box moves every figure alike
            t[k].append(timed_us(f, a.launches))
    res = {"tool": "tools/bench_long_f32_taps.py", "device": torch.cuda.get_device_name(0), "frames": B, "seq_len": S,
           "launches_per_round": a.launches, "rounds": a.rounds, "unit": "us per call",
           "blobs": {"E64": "synth.float_params(64, E=64), one layer, ITAW0003", "E128": "synth.float_params(128, E=128, num_layers=2, tail=False), ITAW0003"},
           "parent_build": bool(a.parent_so),
           "figures": {k: {**stats(v), "bytes_written": nbytes[k],
                           "ratio_to_mha_long_f32": round(float(np.median(v)) / float(np.median(t["mha_long_f32_E" + k.rsplit("_E", 1)[1]])), 3)}
                       for k, v in t.items()}}
    for item in keep:
        item[0].close()
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
