#!/usr/bin/env python3
"""Golden vectors of the MULTI-HEAD int8 attention, by running the reference in the build container (like
tools/gen_golden.py, whose helpers this imports: never on the GPU box).

The reference's model files construct their attention blocks with one head (``self.H = 1``), but
ITASelfAttention_QAT.forward (models/ITA/QAT/layers.py:101-127) reads the block's ``num_heads`` / ``head_dim``
attributes.  They are set on the instance before prepare_qat; everything else is gen_golden's flow: the seeded synthetic
parameters, qconfig on the attention / FFN blocks, calibration forwards, convert, the validation harness's matmul2.
matmul1 and matmul2 stay ONE QFunctional each, so all heads share one logit scale and one context scale.

    heads_E64_H{2,3,4,6}_s0_B{B}.npz   the whole ITAViTLSTM graph (gen_golden.gen_vitlstm's keys, plus meta.H);
                                       logits (s0.attn0.probs.in) and probs are (B, H, 128, 128)
    heads2l_E128_H4_s0_B{B}.npz        models/ITA/QAT/model.py, two layers (gen_golden.gen_vit2l's keys, plus meta.H)

One frame per file (--batch 1).  A fixture may be no larger than the largest one there was before these (1 202 821 B,
vit2l_us_E128_s1_B2.npz).  With two frames the files come to 1 192 709 B (H = 2), 1 226 589 (H = 3), 1 263 906 (H = 4),
1 316 326 (H = 6) and 1 228 772 (E = 128, H = 4): all but the first are over, through the per-head logits and probs, and one
batch size for the whole set keeps the tests uniform.  With one frame they are 633 015 to 786 572 B.
Only DATA is written.  Usage:  python tools/gen_heads_golden.py [--out tests/golden]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as gg  # noqa: E402

synth = gg.synth


def set_heads(blocks, H):
    for blk in blocks:
        P = blk.q_proj.out_features
        assert P % H == 0
        blk.num_heads, blk.head_dim = H, P // H


def _convert(model, calib_seed):
    model.attention_blocks.qconfig = gg.ita_symmetric_qconfig
    model.ffn_blocks.qconfig = gg.ita_symmetric_qconfig
    prepared = torch.ao.quantization.prepare_qat(model.train())
    prepared.lstm.dropout = 0.0
    with torch.no_grad():
        for it in range(4):
            prepared(gg.to_X(synth.frames(calib_seed + it, 8, gain=0.8)))
    conv = torch.ao.quantization.convert(prepared.eval())
    for blk in conv.attention_blocks:
        blk.matmul2.matmul = gg.patched_matmul2(blk.matmul2.scale, blk.matmul2.zero_point)
    return conv


def _two_steps(conv, tap, fr0, fr1):
    with torch.no_grad():
        vel0, (h0, c0) = conv(gg.to_X(fr0, None))
        stage = dict(tap.t)
        vel1, (h1, c1) = conv(gg.to_X(fr1, (h0, c0)))
    rec = {}
    for k, v in fr0.items():
        rec["in0." + k] = v
    for k, v in fr1.items():
        rec["in1." + k] = v
    rec["s0.vel"] = vel0.numpy(); rec["s0.h"] = h0.numpy(); rec["s0.c"] = c0.numpy()
    rec["s1.vel"] = vel1.numpy(); rec["s1.h"] = h1.numpy(); rec["s1.c"] = c1.numpy()
    return stage, rec


def gen_heads_vitlstm(seed, B, H, out_dir):
    """gen_golden.gen_vitlstm with H heads: same parameters, calibration frames, inputs and keys"""
    fp = synth.float_params(seed, E=64)
    model = gg.ITALSTMNetVIT_QAT(num_layers=1)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in fp.items()}, strict=True)
    set_heads(model.attention_blocks, H)
    conv = _convert(model, 100 * seed + 50)
    assert conv.attention_blocks[0].num_heads == H
    tap = gg.Tap()
    tap.add(conv.tokenizer.conv, "tok.conv")
    tap.add(conv.tokenizer, "tok.out")
    gg.tap_attention(tap, conv.attention_blocks[0], "attn0.")
    gg.tap_ffn(tap, conv.ffn_blocks[0], "ffn0.")
    tap.add(conv.norms1[0], "x1")
    tap.add(conv.norms2[0], "x2")
    tap.add(conv.pxShuffle, "tail.shuffled")
    tap.add(conv.up_sample, "tail.upsampled")
    tap.add(conv.down_sample, "tail.conv")
    tap.add(conv.decoder, "dec")
    stage, io = _two_steps(conv, tap, synth.frames(10 * seed, B), synth.frames(10 * seed + 1, B))
    assert stage["attn0.probs"].shape == (B, H, 128, 128) and stage["attn0.out_q.in"].shape == (B, 128, 192)
    rec = {"meta.seed": np.int64(seed), "meta.B": np.int64(B), "meta.E": np.int64(64), "meta.H": np.int64(H),
           "meta.params_sha256": np.array(synth.digest(fp)),
           "meta.torch": np.array(torch.__version__), "meta.engine": np.array("qnnpack")}
    rec.update(gg.block_quant_record("attn0.", attn=conv.attention_blocks[0]))
    rec.update(gg.block_quant_record("ffn0.", ffn=conv.ffn_blocks[0]))
    rec.update(io)
    for k, v in stage.items():
        rec["s0." + k] = v
    rec.pop("s0.tok.conv", None)
    path = os.path.join(out_dir, f"heads_E64_H{H}_s{seed}_B{B}.npz")
    np.savez_compressed(path, **rec)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")


def gen_heads_vit2l(seed, B, H, out_dir):
    """gen_golden.gen_vit2l (models/ITA/QAT/model.py, E = 128, two layers, no fusion tail) with H heads"""
    from models.ITA.QAT.model import ITALSTMNetVIT_QAT as ITAViT2L
    fp = synth.float_params(seed, E=128, num_layers=2, tail=False)
    model = ITAViT2L()
    ren = lambda k: k.replace("norms1.", "norm1_layers.").replace("norms2.", "norm2_layers.")
    model.load_state_dict({ren(k): torch.from_numpy(v) for k, v in fp.items()}, strict=True)
    set_heads(model.attention_blocks, H)
    conv = _convert(model, 100 * seed + 70)
    tap = gg.Tap()
    tap.add(conv.tokenizer, "tok.out")
    for i in range(2):
        gg.tap_attention(tap, conv.attention_blocks[i], f"attn{i}.")
        gg.tap_ffn(tap, conv.ffn_blocks[i], f"ffn{i}.")
        tap.add(conv.norm1_layers[i], f"x1_{i}")
        tap.add(conv.norm2_layers[i], f"x2_{i}")
    tap.add(conv.decoder, "dec")
    stage, io = _two_steps(conv, tap, synth.frames(10 * seed + 5, B), synth.frames(10 * seed + 6, B))
    assert stage["attn1.probs"].shape == (B, H, 128, 128)
    rec = {"meta.seed": np.int64(seed), "meta.B": np.int64(B), "meta.E": np.int64(128), "meta.num_layers": np.int64(2),
           "meta.H": np.int64(H), "meta.params_sha256": np.array(synth.digest(fp)),
           "meta.torch": np.array(torch.__version__), "meta.engine": np.array("qnnpack")}
    for i in range(2):
        rec.update(gg.block_quant_record(f"attn{i}.", attn=conv.attention_blocks[i]))
        rec.update(gg.block_quant_record(f"ffn{i}.", ffn=conv.ffn_blocks[i]))
    rec.update(io)
    for k in ("tok.out", "x1_0", "x2_0", "x1_1", "x2_1", "dec", "attn0.x_q", "attn0.out_q", "ffn0.out_q", "attn1.x_q",
              "attn1.probs", "attn1.out_q", "ffn1.h1_relu", "ffn1.out_q"):
        rec["s0." + k] = stage[k]
    path = os.path.join(out_dir, f"heads2l_E128_H{H}_s{seed}_B{B}.npz")
    np.savez_compressed(path, **rec)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(gg.REPO, "tests", "golden"))
    ap.add_argument("--batch", type=int, default=1, help="frames per fixture (with two, four of the five files exceed the largest "
                                                         "fixture there was before: see the module docstring)")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    for H in (2, 3, 4, 6):
        gen_heads_vitlstm(0, a.batch, H, a.out)
    gen_heads_vit2l(0, a.batch, 4, a.out)


if __name__ == "__main__":
    main()
