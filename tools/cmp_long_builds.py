#!/usr/bin/env python3
"""Two builds of the library on the same long-sequence inputs, byte for byte (GPU box).

This build's libita_mi355x.so and another build of it (--other-so, for instance the commit before a refactor of the long
kernels) are loaded into one process, each with its own handle and weights, and every long attention entry runs on both:

  int8    ita_mha_long_q8, ita_mha_long_int8, ita_mha_long_int8_taps (every tap, 16 rows), ita_mha_long_int8_stats (all six)
          on four fixtures: E = 64 and E = 128, each in the FAST and in the exact requantisation form
  float   ita_mha_long_f32, ita_mha_long_f32_taps (every tap, 16 rows), ita_mha_long_f32_stats (all six, p_min = 1 / 256)
          on the ITAW0003 blobs of tools/bench_long_f32.py at E = 64 and E = 128

at B = 2 frames and S = 128 and 384 tokens (one and three query tiles, both parities of the K ring).  Every output buffer
starts from the same canary bytes in both runs and is compared as bytes.  Prints one line per (blob, S, entry) and exits
with status 1 if any byte differs.  Takes seconds.  Not a pytest test: the other build is not part of the tree.
usage: python tools/cmp_long_builds.py --other-so PATH [--out profiles/long_shared_bits.txt]"""
import argparse, ctypes as C, math, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from drone_oa_iree_vit_accelerator_amd import host, params, synth

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
INT8_FIXTURES = ("vitlstm_E64_seed0_B2", "vitlstm_E64_seed1_B2", "vit2l_us_E128_s1_B2", "blocks_E128_seed0_B1")
B, SEQS, P, NROWS = 2, (128, 384), 192, 16
vp, ci = C.c_void_p, C.c_int


class Build:
    """one build of the library through its C ABI: a handle with the blob loaded"""

    def __init__(self, so, blob):
        L = self.lib = C.CDLL(os.path.abspath(so))
        L.ita_create.argtypes = [C.POINTER(vp), ci]
        L.ita_destroy.argtypes = [vp]
        L.ita_load_weights.argtypes = [vp, vp, C.c_size_t]
        L.ita_error_string.restype = C.c_char_p
        L.ita_debug_layer_forms.argtypes = [vp, ci, C.POINTER(C.c_uint), C.POINTER(ci)]
        L.ita_mha_long_q8.argtypes = [vp, ci, vp, vp, ci, ci, vp]
        L.ita_mha_long_int8.argtypes = [vp, ci, vp, vp, ci, ci, vp]
        L.ita_mha_long_int8_taps.argtypes = [vp, ci, vp, vp, ci, ci, C.POINTER(host._MhaLongTaps), vp]
        L.ita_mha_long_int8_stats.argtypes = [vp, ci, vp, ci, ci, C.POINTER(host._MhaLongStats), vp]
        L.ita_mha_long_f32.argtypes = [vp, ci, vp, vp, ci, ci, vp]
        L.ita_mha_long_f32_taps.argtypes = [vp, ci, vp, vp, ci, ci, C.POINTER(host._MhaLongF32Taps), vp]
        L.ita_mha_long_f32_stats.argtypes = [vp, ci, vp, ci, ci, C.c_float, C.POINTER(host._MhaLongF32Stats), vp]
        self.so, self.h = so, vp()
        self.chk(L.ita_create(C.byref(self.h), 0))
        self.chk(L.ita_load_weights(self.h, C.create_string_buffer(blob, len(blob)), len(blob)))

    def chk(self, rc):
        if rc:
            raise SystemExit(f"{self.so}: ita status {rc}: {self.lib.ita_error_string().decode()}")

    def fast(self):
        m, im = C.c_uint(0), ci(0)
        self.chk(self.lib.ita_debug_layer_forms(self.h, 0, C.byref(m), C.byref(im)))
        return m.value == 63

    def close(self):
        self.lib.ita_destroy(self.h)


def int8_blob(name):
    """(E, blob, input scale) of a golden fixture, as tests/test_gpu_long_taps.py builds it"""
    d = params.load_fixture(os.path.join(GOLDEN, name + ".npz"))
    E = int(d["meta.E"])
    nl = int(d["meta.num_layers"]) if "meta.num_layers" in d else 1
    fp = synth.float_params(int(d["meta.seed"]), E=E, num_layers=nl, tail=(E == 64)) if name.startswith("vit") else None
    s_x = 1.0 / float(params.attention_tensors(d, "attn0.", 0)["attn0.scal"][0])
    return E, params.blob_from_record(d, fp, E=E, num_layers=nl), s_x


def buffers(spec):
    """{name: tensor} of canary bytes (0xA5) for {name: (shape, dtype)}"""
    def canary(shape, dt):
        nbytes = math.prod(shape) * torch.empty((), dtype=dt).element_size()
        return torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda").view(dt).reshape(shape)
    return {k: canary(s, dt) for k, (s, dt) in spec.items()}


def int8_entries(E, S, x, xq, rows):
    """{entry: (output spec, call(build, outputs))} of the four int8 entries"""
    i8, u8, i32, f32 = torch.int8, torch.uint8, torch.int32, torch.float32
    arr = (ci * NROWS)(*rows)
    taps = dict(x_q=((B, S, E), i8), Q=((B, S, P), i8), K=((B, S, P), i8), V=((B, S, P), i8), ctx=((B, S, P), i8),
                out_q=((B, S, E), i8), logits=((B, NROWS, S), i8), probs=((B, NROWS, S), u8), row_max=((B, NROWS), i8),
                row_sum=((B, NROWS), i32))
    stats = {k: ((B, S), i8 if k == "row_max" else i32) for k in host.LONG_STATS}

    def run_taps(b, o):
        st = host._MhaLongTaps(**{k: o[k].data_ptr() for k in taps})
        st.rows, st.n_rows = arr, NROWS
        b.chk(b.lib.ita_mha_long_int8_taps(b.h, 0, x.data_ptr(), o["y"].data_ptr(), B, S, C.byref(st), None))

    def run_stats(b, o):
        st = host._MhaLongStats(**{k: o[k].data_ptr() for k in stats})
        b.chk(b.lib.ita_mha_long_int8_stats(b.h, 0, x.data_ptr(), B, S, C.byref(st), None))

    return {
        "ita_mha_long_q8": ({"out_q": ((B, S, E), i8)},
                            lambda b, o: b.chk(b.lib.ita_mha_long_q8(b.h, 0, xq.data_ptr(), o["out_q"].data_ptr(), B, S, None))),
        "ita_mha_long_int8": ({"y": ((B, S, E), f32)},
                              lambda b, o: b.chk(b.lib.ita_mha_long_int8(b.h, 0, x.data_ptr(), o["y"].data_ptr(), B, S, None))),
        "ita_mha_long_int8_taps": ({"y": ((B, S, E), f32), **taps}, run_taps),
        "ita_mha_long_int8_stats": (stats, run_stats),
    }


def f32_entries(E, S, x, rows):
    """{entry: (output spec, call(build, outputs))} of the three float entries"""
    i32, f32 = torch.int32, torch.float32
    arr = (ci * NROWS)(*rows)
    taps = dict(Q=((B, S, P), f32), K=((B, S, P), f32), V=((B, S, P), f32), ctx=((B, S, P), f32), logits=((B, NROWS, S), f32),
                probs=((B, NROWS, S), f32), row_max=((B, NROWS), f32), row_sum=((B, NROWS), f32))
    stats = {k: ((B, S), i32 if k.endswith("_nnz") else f32) for k in host.LONG_F32_STATS}

    def run_taps(b, o):
        st = host._MhaLongF32Taps(**{k: o[k].data_ptr() for k in taps})
        st.rows, st.n_rows = arr, NROWS
        b.chk(b.lib.ita_mha_long_f32_taps(b.h, 0, x.data_ptr(), o["y"].data_ptr(), B, S, C.byref(st), None))

    def run_stats(b, o):
        st = host._MhaLongF32Stats(**{k: o[k].data_ptr() for k in stats})
        b.chk(b.lib.ita_mha_long_f32_stats(b.h, 0, x.data_ptr(), B, S, 1.0 / 256, C.byref(st), None))

    return {
        "ita_mha_long_f32": ({"y": ((B, S, E), f32)},
                             lambda b, o: b.chk(b.lib.ita_mha_long_f32(b.h, 0, x.data_ptr(), o["y"].data_ptr(), B, S, None))),
        "ita_mha_long_f32_taps": ({"y": ((B, S, E), f32), **taps}, run_taps),
        "ita_mha_long_f32_stats": (stats, run_stats),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other-so", required=True)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cmp_long_builds.py runs on the GPU: none visible")
    this_so = host.build_extension()
    lines = [f"tools/cmp_long_builds.py: this build against the build given as --other-so, B = {B}, S in {SEQS}, "
             f"device {torch.cuda.get_device_name(0)}"]
    differ = 0

    def compare(label, blob, entries_of, int8):
        nonlocal differ
        builds = [Build(this_so, blob), Build(a.other_so, blob)]
        form = ""
        if int8:
            form = " FAST" if builds[0].fast() else " exact"
            assert builds[0].fast() == builds[1].fast()
        for S in SEQS:
            for entry, (spec, call) in entries_of(S).items():
                outs = []
                for b in builds:
                    o = buffers(spec)
                    call(b, o)
                    torch.cuda.synchronize()
                    outs.append(o)
                bad = [k for k in spec if not torch.equal(outs[0][k].reshape(-1).view(torch.uint8), outs[1][k].reshape(-1).view(torch.uint8))]
                nbytes = sum(v.numel() * v.element_size() for v in outs[0].values())
                differ += len(bad)
                lines.append(f"{label + form:32s} S = {S:3d}  {entry:24s} " +
                             (f"DIFFERENT in {', '.join(bad)}" if bad else f"identical: {len(spec)} outputs, {nbytes} bytes"))
        for b in builds:
            b.close()

    g = torch.Generator(device="cpu").manual_seed(11)
    for name in INT8_FIXTURES:
        E, blob, s_x = int8_blob(name)

        def int8_entries_for(S, E=E, s_x=s_x):
            # structured rows (tools/bench_long_layer.py): groups of similar tokens, so that the softmax rows are not flat
            base = torch.randn((B, S // 32, E), generator=g).repeat_interleave(32, dim=1) * 18.0
            xq = (base + torch.randn((B, S, E), generator=g) * 9.0).round().clamp(-128, 127)
            x = ((xq + (torch.rand((B, S, E), generator=g) - 0.5) * 0.8) * s_x).cuda()
            return int8_entries(E, S, x, xq.to(torch.int8).cuda(), list(range(0, S, S // NROWS)))

        compare(f"{name} E = {E}", blob, int8_entries_for, True)
    for E in (64, 128):
        L = 1 if E == 64 else 2
        blob = params.blob_from_float_params(synth.float_params(E, E=E, num_layers=L, tail=(E == 64)), L)

        def f32_entries_for(S, E=E):
            x = torch.randn((B, S, E), generator=g)     # LayerNorm-like rows, as tools/bench_long_f32.py builds them
            x = ((x - x.mean(-1, keepdim=True)) / x.std(-1, keepdim=True, unbiased=False)).cuda()
            return f32_entries(E, S, x, list(range(0, S, S // NROWS)))

        compare(f"ITAW0003 float E = {E}", blob, f32_entries_for, False)
    lines.append("RESULT: " + (f"{differ} outputs differ" if differ else "every output of every entry is byte-identical in the two builds"))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    sys.exit(1 if differ else 0)


if __name__ == "__main__":
    main()
