#!/usr/bin/env python3
"""Fixtures for the wire ingest: the reference host's own resize, RUN in the build container, on generated frames.

Runs only where the reference checkout exists (ITA_REFERENCE_ROOT, default /root/reference; never on the GPU box).  It
writes a few-line C driver of its own into a temporary directory, compiles it against the reference's vendored
stb_image_resize2.h with plain `gcc -O2` (the build samples/utils/libs.cpp gets: x86-64 defaults, no FMA define), runs it
-- stbir_resize_uint8_linear(src, W, H, 0, dst, 90, 60, 0, STBIR_1CHANNEL), the call of
samples/inference_trainingset_custom_dispatch/main.cpp:117-128 -- and stores inputs, stb's output codes and the compiler
line in tests/golden/resize_stb_<H>x<W>.npz.  Only DATA is written: neither the binary nor any text of the header.

Five frames per size: uniform noise, a smooth field, flat blocks with edges, all-255, 0/255 noise.  The large sizes use
block noise so that every file stays well under the size limit for a committed file.

Usage:  python tools/gen_resize_golden.py [--out tests/golden]
"""
import argparse
import os
import subprocess
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("ITA_REFERENCE_ROOT", "/root/reference")

# (H, W, side of the noise blocks): 1 = per-pixel noise
SIZES = [(96, 128, 1), (480, 640, 1), (720, 1280, 4), (61, 93, 1), (30, 45, 1), (100, 64, 1), (1, 200, 1), (200, 1, 1),
         (1, 1, 1), (8, 4096, 1), (4096, 8, 1)]

DRIVER = r"""
#define STB_IMAGE_RESIZE_IMPLEMENTATION
#include "stb_image_resize2.h"
#include <stdio.h>
#include <stdlib.h>
int main(int argc, char** argv) {
  int h = atoi(argv[1]), w = atoi(argv[2]), n = atoi(argv[3]);
  unsigned char* src = (unsigned char*)malloc((size_t)h * w);
  unsigned char dst[60 * 90];
  FILE* in = fopen(argv[4], "rb");
  FILE* out = fopen(argv[5], "wb");
  for (int k = 0; k < n; ++k) {
    if (fread(src, 1, (size_t)h * w, in) != (size_t)h * w) return 2;
    if (!stbir_resize_uint8_linear(src, w, h, 0, dst, 90, 60, 0, STBIR_1CHANNEL)) return 3;
    fwrite(dst, 1, sizeof dst, out);
  }
  fclose(out);
  return 0;
}
"""


def _blocky(rs, H, W, side, values):
    small = values(rs, ((H + side - 1) // side, (W + side - 1) // side))
    return np.kron(small, np.ones((side, side), np.uint8))[:H, :W]


def frames(H, W, side):
    rs = np.random.RandomState(H * 8191 + W)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    noise = _blocky(rs, H, W, side, lambda r, s: r.randint(0, 256, size=s).astype(np.uint8))
    field = np.rint(127.5 + 127.5 * np.sin(yy / max(H, 2) * 5.1 + 0.3) * np.cos(xx / max(W, 2) * 7.3 + 0.1)).astype(np.uint8)
    # block levels 62 apart, an EVEN step: an output pixel centred on a block edge gets the exact mean of the two levels,
    # and with an odd step mean + 0.5 is an integer -- a tie of the final truncation built into the picture, repeated
    # along every edge, at which any two correct float32 summations may land on either side
    flat = _blocky(rs, H, W, max(side, 1) * 16, lambda r, s: (r.randint(0, 5, size=s) * 62).astype(np.uint8))
    white = np.full((H, W), 255, np.uint8)
    binary = _blocky(rs, H, W, side, lambda r, s: (r.randint(0, 2, size=s) * 255).astype(np.uint8))
    return np.stack([noise, field, flat, white, binary])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    args = ap.parse_args()
    inc = os.path.join(REF, "samples", "utils", "include")
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "driver.c"), os.path.join(tmp, "driver")
        with open(src, "w") as f:
            f.write(DRIVER)
        cc = ["gcc", "-O2", "-I", inc, src, "-o", exe, "-lm"]
        subprocess.check_call(cc)
        cc_line = " ".join(["gcc", "-O2", "-I", "<reference>/samples/utils/include", "driver.c", "-o", "driver", "-lm"])
        for H, W, side in SIZES:
            x = frames(H, W, side)
            fin, fout = os.path.join(tmp, "in.raw"), os.path.join(tmp, "out.raw")
            x.tofile(fin)
            subprocess.check_call([exe, str(H), str(W), str(len(x)), fin, fout])
            y = np.fromfile(fout, np.uint8).reshape(len(x), 60, 90)
            path = os.path.join(args.out, f"resize_stb_{H}x{W}.npz")
            np.savez_compressed(path, src=x, stb=y, compiler=np.array(cc_line),
                                kinds=np.array(["noise", "field", "flat", "white", "binary"]))
            print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
