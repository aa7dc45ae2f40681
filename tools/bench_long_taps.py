#!/usr/bin/env python3
"""Cost of the long-sequence taps (GPU box): 32 frames of S = 8192 tokens, E = 64 (vitlstm_E64_seed0: the FAST form) and
E = 128 (vit2l_E128_s0: the exact form), the blobs and inputs of tools/bench_long_layer.py.

  mha_long          ita_mha_long_int8 of this build (the production kernels)
  mha_long_parent   the same entry of another build of the library (--parent-so: the commit before the taps), loaded
                    beside this one in the same process and timed in the same rounds
  taps_null         ita_mha_long_int8_taps with every tap NULL: the taps kernels, no extra store
  taps_probs16      the same with probs for 16 query rows
  taps_tensors      the same with the six stage tensors (x_q, Q, K, V, ctx, out_q), no rows

Device events around --launches calls after a warm-up, --rounds rounds with the figures interleaved; min / median / max
per figure, and the bytes each variant writes (y and the taps; the workspace traffic is the same for all).
usage: python tools/bench_long_taps.py [--out profiles/long_taps.json] [--parent-so PATH] [--frames 32] [--seq 8192]
[--launches 10] [--rounds 5]"""
import argparse, ctypes as C, json, os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from drone_oa_iree_vit_accelerator_amd import host
from bench_long_layer import blob_of, stats, timed_us


class OtherBuild:
    """ita_mha_long_int8 of another build of the library: its own handle and weights"""

    def __init__(self, so, blob):
        self.lib = C.CDLL(os.path.abspath(so))
        vp, i = C.c_void_p, C.c_int
        self.lib.ita_create.argtypes = [C.POINTER(vp), i]
        self.lib.ita_destroy.argtypes = [vp]
        self.lib.ita_load_weights.argtypes = [vp, vp, C.c_size_t]
        self.lib.ita_mha_long_int8.argtypes = [vp, i, vp, vp, i, i, vp]
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
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_long_taps.py measures on the GPU: none visible")
    B, S, lib, P = a.frames, a.seq, host.lib(), 192
    fns, nbytes, keep = {}, {}, []
    for E in (128, 64):
        blob, s_x = blob_of(E)
        eng = host.Engine(blob, device=0)
        g = torch.Generator(device="cpu").manual_seed(5 + E)      # structured rows, as bench_long_layer.py builds them
        base = torch.randn((B, S // 32, E), generator=g).repeat_interleave(32, dim=1) * 18.0
        xq = (base + torch.randn((B, S, E), generator=g) * 9.0).round().clamp(-128, 127)
        x = ((xq + (torch.rand((B, S, E), generator=g) - 0.5) * 0.8) * s_x).cuda()
        y, sp = torch.empty_like(x), host._stream_ptr(0)
        rows = list(range(0, S, S // 16))[:16]
        arr = (C.c_int * 16)(*rows)
        mk = lambda *s, dt=torch.int8: torch.empty(s, dtype=dt, device="cuda")
        probs = mk(B, 16, S, dt=torch.uint8)
        tens = dict(x_q=mk(B, S, E), out_q=mk(B, S, E), Q=mk(B, S, P), K=mk(B, S, P), V=mk(B, S, P), ctx=mk(B, S, P))
        st_null = host._MhaLongTaps()
        st_probs = host._MhaLongTaps(probs=probs.data_ptr())
        st_probs.rows, st_probs.n_rows = arr, 16
        st_tens = host._MhaLongTaps(**{k: v.data_ptr() for k, v in tens.items()})
        keep.append((eng, x, y, arr, probs, tens))

        def mha(eng=eng, x=x, y=y, sp=sp):
            host._chk(lib.ita_mha_long_int8(eng._h, 0, x.data_ptr(), y.data_ptr(), B, S, sp))

        def taps(st, eng=eng, x=x, y=y, sp=sp):
            return lambda: host._chk(lib.ita_mha_long_int8_taps(eng._h, 0, x.data_ptr(), y.data_ptr(), B, S, C.byref(st), sp))

        ybytes = B * S * E * 4
        fns[f"mha_long_E{E}"], nbytes[f"mha_long_E{E}"] = mha, ybytes
        if a.parent_so:
            other = OtherBuild(a.parent_so, blob)
            keep.append((other,))

            def parent(other=other, x=x, y=y, sp=sp):
                other.chk(other.lib.ita_mha_long_int8(other.h, 0, x.data_ptr(), y.data_ptr(), B, S, sp))
            fns[f"mha_long_parent_E{E}"], nbytes[f"mha_long_parent_E{E}"] = parent, ybytes
        fns[f"taps_null_E{E}"], nbytes[f"taps_null_E{E}"] = taps(st_null), ybytes
        fns[f"taps_probs16_E{E}"], nbytes[f"taps_probs16_E{E}"] = taps(st_probs), ybytes + B * 16 * S
        fns[f"taps_tensors_E{E}"], nbytes[f"taps_tensors_E{E}"] = taps(st_tens), ybytes + 2 * B * S * E + 4 * B * S * P
    for f in fns.values():
        for _ in range(2):
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(a.rounds):
        for k, f in fns.items():       # interleaved: a drift of the box moves every figure alike
            t[k].append(timed_us(f, a.launches))
    res = {"tool": "tools/bench_long_taps.py", "device": torch.cuda.get_device_name(0), "frames": B, "seq_len": S,
           "launches_per_round": a.launches, "rounds": a.rounds, "unit": "us per call",
           "blobs": {"E64": "vitlstm_E64_seed0_B2 (one layer, FAST form)", "E128": "vit2l_E128_s0_B2 (two layers, exact form)"},
           "parent_build": bool(a.parent_so),
           "figures": {k: {**stats(v), "bytes_written": nbytes[k],
                           "ratio_to_mha_long": round(float(np.median(v)) / float(np.median(t["mha_long_E" + k.rsplit("_E", 1)[1]])), 3)}
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
