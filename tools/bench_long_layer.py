#!/usr/bin/env python3
"""Cost of the long-sequence encoder layer (GPU box): S = 8192 tokens per frame, 32 frames, E = 64 (vitlstm_E64_seed0: the
FAST requantisation form) and E = 128 (vit2l_E128_s0, two layers: the exact form).

  q8          ita_mha_long_q8: int8 codes in and out.  At E = 128 this is the path that existed before the f32 forms and
              the baseline every other figure is set against (ratio_to_q8_E128)
  mha_long    ita_mha_long_int8: f32 in (quantised in the projection kernel), f32 out (dequantised in the attention kernel)
  layer       ita_encoder_layer_long: the two long launches with residual + LayerNorm1, then the FFN block kernel with
              residual + LayerNorm2 in place
  layer_ffn   the layer's FFN part alone: ita_ffn_int8 over the same rows as batch * S / 128 blocks (the same kernel
              without residual + LayerNorm2); the layer's attention part is mha_long plus the LayerNorm1 epilogue
  c5_chain    (E = 128) encode_long over both layers, then ita_fusion_tail_large on the 64 x 128 token grid, 48 outputs

Device events around --launches calls after a warm-up, --rounds rounds with the figures interleaved; min / median / max
per figure.  usage: python tools/bench_long_layer.py [--out profiles/long_layer.json] [--frames 32] [--seq 8192]
[--launches 10] [--rounds 5]"""
import argparse, json, os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from drone_oa_iree_vit_accelerator_amd import host, params, synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")


def blob_of(E):
    if E == 64:
        d, nl = params.load_fixture(os.path.join(GOLDEN, "vitlstm_E64_seed0_B2.npz")), 1
        fp = synth.float_params(0, E=64)
    else:
        d, nl = params.load_fixture(os.path.join(GOLDEN, "vit2l_E128_s0_B2.npz")), 2
        fp = synth.float_params(0, E=128, num_layers=2, tail=False)
    s_x = 1.0 / float(params.attention_tensors(d, "attn0.", 0)["attn0.scal"][0])
    return params.blob_from_record(d, fp, E=E, num_layers=nl), s_x


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
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_long_layer.py measures on the GPU: none visible")
    B, S, lib = a.frames, a.seq, host.lib()
    th, tw, co = 64, S // 64, 48
    fns, keep = {}, []
    for E in (128, 64):
        blob, s_x = blob_of(E)
        eng = host.Engine(blob, device=0)
        g = torch.Generator(device="cpu").manual_seed(5 + E)      # structured rows, as bench.py's c5_mha builds them
        base = torch.randn((B, S // 32, E), generator=g).repeat_interleave(32, dim=1) * 18.0
        xq = (base + torch.randn((B, S, E), generator=g) * 9.0).round().clamp(-128, 127).to(torch.int8).cuda()
        x = (xq.float() + (torch.rand((B, S, E), generator=g).cuda() - 0.5) * 0.8) * s_x
        yq, y = torch.empty_like(xq), torch.empty_like(x)
        x1 = eng.encoder_layer_long(x, 0)                          # LayerNorm-like rows for the FFN part
        sp = host._stream_ptr(0)
        keep.append((eng, xq, x, yq, y, x1))

        def q8(eng=eng, xq=xq, yq=yq, sp=sp):
            host._chk(lib.ita_mha_long_q8(eng._h, 0, xq.data_ptr(), yq.data_ptr(), B, S, sp))

        def mha(eng=eng, x=x, y=y, sp=sp):
            host._chk(lib.ita_mha_long_int8(eng._h, 0, x.data_ptr(), y.data_ptr(), B, S, sp))

        def layer(eng=eng, x=x, y=y):
            eng.encoder_layer_long(x, 0, out=y)

        def ffn(eng=eng, x1=x1, y=y, sp=sp):
            host._chk(lib.ita_ffn_int8(eng._h, 0, x1.data_ptr(), y.data_ptr(), B * (S // 128), sp))

        fns.update({f"q8_E{E}": q8, f"mha_long_E{E}": mha, f"layer_E{E}": layer, f"layer_ffn_E{E}": ffn})
        if E == 128:
            c = synth.tail_large_case(0, E, th, tw, co, 1)
            tail = host.FusionTailLarge(c["conv_w"], c["conv_b"], device=0)
            fmap = torch.empty((B, co, 2 * th, 2 * tw), device="cuda")
            keep.append((tail, fmap))

            def chain(eng=eng, x=x, tail=tail, fmap=fmap):
                tail(eng.encode_long(x), th, tw, out=fmap)

            def chain_tail(tail=tail, y=y, fmap=fmap):
                tail(y, th, tw, out=fmap)
            fns.update({"c5_chain_E128": chain, "c5_chain_tail_E128": chain_tail})
    for f in fns.values():
        for _ in range(2):
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(a.rounds):
        for k, f in fns.items():       # interleaved: a drift of the box moves every figure alike
            t[k].append(timed_us(f, a.launches))
    base = float(np.median(t["q8_E128"]))
    res = {"tool": "tools/bench_long_layer.py", "device": torch.cuda.get_device_name(0), "frames": B, "seq_len": S,
           "launches_per_round": a.launches, "rounds": a.rounds, "unit": "us per call",
           "blobs": {"E64": "vitlstm_E64_seed0_B2 (one layer, FAST form)", "E128": "vit2l_E128_s0_B2 (two layers, exact form)"},
           "figures": {k: {**stats(v), "ratio_to_q8_E128": round(float(np.median(v)) / base, 3),
                           "frames_per_s": round(B / float(np.median(v)) * 1e6, 1)} for k, v in t.items()}}
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
