#!/usr/bin/env python3
"""Cost of attention heads on the block route (GPU box): at 1024 frames, E = 64 (ITAViTLSTM, one layer) and E = 128 (two
layers, no fusion tail), the attention launch ita_mha_kernel<E, H> for H = 1, 2, 3, 4, 6 and the whole step of each blob.

The weights do not depend on H, so one record per E is packed with each head count.  H = 1 is timed on the same block kernel
(ita_mha_int8_taps with an all-NULL tap struct selects it; without taps a one-head layer runs the stream kernel), which
is the baseline the heads are compared with; the H = 1 step is the stream-kernel step a one-head blob really runs.

Device events around --launches launches after a warm-up, --rounds rounds with the head counts interleaved; min / median /
max per figure.  usage: python tools/bench_heads.py [--out profiles/heads.json] [--frames 1024] [--launches 200] [--rounds 5]"""
import argparse, ctypes, json, os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from drone_oa_iree_vit_accelerator_amd import host, params, synth

HEADS = (1, 2, 3, 4, 6)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")


def blob_of(E, H):
    if E == 64:
        d, fp, nl = params.load_fixture(os.path.join(GOLDEN, "vitlstm_E64_seed0_B2.npz")), synth.float_params(0, E=64), 1
    else:
        d, nl = params.load_fixture(os.path.join(GOLDEN, "vit2l_E128_s0_B2.npz")), 2
        fp = synth.float_params(0, E=128, num_layers=2, tail=False)
    return params.blob_from_record(d, fp, E=E, num_layers=nl, H=H)


def timed_us(fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / launches


def stats(v):
    return {"min": round(min(v), 3), "median": round(float(np.median(v)), 3), "max": round(max(v), 3), "rounds": [round(x, 3) for x in v]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_heads.py measures on the GPU: none visible")
    B, lib = a.frames, host.lib()
    res = {"tool": "tools/bench_heads.py", "device": torch.cuda.get_device_name(0), "frames": B, "launches_per_round": a.launches,
           "rounds": a.rounds, "unit": "us", "E": {}}
    fr = synth.frames(11, B)
    img, dv, qt = (torch.from_numpy(fr[k]).cuda() for k in ("img_u8", "desvel", "quat"))
    for E in (64, 128):
        x = torch.from_numpy(np.random.RandomState(E).standard_normal((B, 128, E)).astype(np.float32)).cuda()
        y = torch.empty_like(x)
        no_taps = host._MhaTaps()
        state = [(torch.zeros((3, B, 128), device="cuda"), torch.zeros((3, B, 128), device="cuda")) for _ in range(2)]
        vel = torch.empty((B, 3), device="cuda")
        engines, fns = {}, {}
        for H in HEADS:
            eng = engines[H] = host.Engine(blob_of(E, H), device=0, reserve=B)
            sp = host._stream_ptr(0)

            def attn(eng=eng, sp=sp):
                host._chk(lib.ita_mha_int8_taps(eng._h, 0, x.data_ptr(), y.data_ptr(), B, ctypes.byref(no_taps), sp))

            def step(eng=eng, i=[0]):
                eng.forward(img, dv, qt, state[i[0] & 1], out=(vel, *state[(i[0] + 1) & 1]))
                i[0] += 1
            fns[H] = (attn, step)
            for f in fns[H]:
                for _ in range(20):
                    f()
        torch.cuda.synchronize()
        t = {H: ([], []) for H in HEADS}
        for _ in range(a.rounds):
            for H in HEADS:            # interleaved: a drift of the box moves every head count alike
                for k in (0, 1):
                    t[H][k].append(timed_us(fns[H][k], a.launches))
        base = float(np.median(t[1][0]))
        res["E"][str(E)] = {f"H{H}": {"attention_block_kernel_us": stats(t[H][0]),
                                      "attention_over_H1_block_kernel": round(float(np.median(t[H][0])) / base, 3),
                                      "step_us": stats(t[H][1]), "frames_per_s": round(B / float(np.median(t[H][1])) * 1e6),
                                      "step_route": "stream kernel" if H == 1 else "tokenizer + block attention + block FFN per layer"}
                            for H in HEADS}
        for eng in engines.values():
            assert eng.head_status() == 0
            eng.close()
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
