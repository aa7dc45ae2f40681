#!/usr/bin/env python3
"""Golden vectors of the long-sequence tokenizer, by running the reference's own OverlapPatchMerging
(models/ITA/QAT/layers.py:39-45) in the build container (like tools/gen_heads_golden.py: never on the GPU box).  The
module is imported from the reference and constructed with output_size = the token grid; none of it is copied.

    toklong_E{64,128}_{H}x{W}_T{tok_h}x{tok_w}.npz
        img            (1, H, W) float32 in [0, 1)          seeded (numpy legacy RandomState)
        tokens         (1, tok_h * tok_w, E) float32        the reference module's output
        meta.*         E, tok_h, tok_w, seed, params_sha256 (synth.float_params(seed, E)), torch version

Frames and grids: 97 x 131 -> 8 x 16, 20 x 30 -> 8 x 32 (an up-sampling resize: the conv grid is 10 x 15) and
120 x 180 -> 16 x 32, each at E = 64 and E = 128.  The largest file is 321 KB (the largest fixture there was before: 1.2 MB).
Only DATA is written.  Usage:  python tools/gen_tokenizer_long_golden.py [--out tests/golden]
"""
import argparse
import importlib.util
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("ITA_REFERENCE_ROOT", "/root/reference")

spec = importlib.util.spec_from_file_location("ita_synth", os.path.join(REPO, "drone-oa-iree-vit-accelerator_amd", "synth.py"))
synth = importlib.util.module_from_spec(spec)
spec.loader.exec_module(synth)

sys.path.insert(0, REF)
from models.ITA.QAT.layers import OverlapPatchMerging  # noqa: E402

CASES = ((97, 131, 8, 16), (20, 30, 8, 32), (120, 180, 16, 32))
SEED = 0


def image(H, W):
    """a smooth field plus noise, so neighbouring patches differ: (1, H, W) float32 in [0, 1)"""
    rs = np.random.RandomState(7000 + 31 * H + W)
    base = rs.uniform(0, 1, size=((H + 9) // 10, (W + 9) // 10))
    img = np.kron(base, np.ones((10, 10)))[:H, :W] * 0.7 + rs.uniform(0, 1, size=(H, W)) * 0.3
    return np.minimum(img, np.nextafter(np.float32(1), np.float32(0))).astype(np.float32)[None]


def gen(E, H, W, tok_h, tok_w, out_dir):
    fp = synth.float_params(SEED, E=E)
    m = OverlapPatchMerging(1, E, 7, 2, 3, (tok_h, tok_w))
    m.load_state_dict({k[len("tokenizer."):]: torch.from_numpy(v) for k, v in fp.items() if k.startswith("tokenizer.")}, strict=True)
    img = image(H, W)
    with torch.no_grad():
        tok, th, tw = m.eval()(torch.from_numpy(img)[:, None])
    assert (th, tw) == (tok_h, tok_w) and tuple(tok.shape) == (1, tok_h * tok_w, E)
    rec = {"img": img, "tokens": tok.numpy(), "meta.E": np.int64(E), "meta.tok_h": np.int64(tok_h), "meta.tok_w": np.int64(tok_w),
           "meta.seed": np.int64(SEED), "meta.params_sha256": np.array(synth.digest(fp)), "meta.torch": np.array(torch.__version__)}
    path = os.path.join(out_dir, f"toklong_E{E}_{H}x{W}_T{tok_h}x{tok_w}.npz")
    np.savez_compressed(path, **rec)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    torch.manual_seed(0)
    for E in (64, 128):
        for H, W, th, tw in CASES:
            gen(E, H, W, th, tw, a.out)


if __name__ == "__main__":
    main()
