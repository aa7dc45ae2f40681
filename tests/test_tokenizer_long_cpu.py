"""CPU-side checks of the long-sequence tokenizer (tokenizer_long_ref.py, ita_tokenizer_long, Engine.tokenize_long /
encode_frames_long).  The bit-exact expectation is COMPOSED here from the definition's blended patches and two oracle
functions with exactly the chains the definition names:

    oracle.add_ln(oracle.linear_f32(pb.reshape(-1, 49), conv_w.reshape(E, 49), conv_b), 0, ln_w, ln_b)

(linear_f32: one ascending-k fmaf chain started from the bias; add_ln with y = 0: x + 0 = x exactly, then the project's
LayerNorm).  tests/test_gpu_tokenizer_long.py compares the kernel with the same composition.  No GPU call is made here."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from conftest import REPO, golden_files
from drone_oa_iree_vit_accelerator_amd import host, synth
from drone_oa_iree_vit_accelerator_amd import tokenizer_long_ref as tl
from tokenizer_long_common import composed, tok_params

# grids of the fixtures, the GPU test's table and BASELINE config 5
GRIDS = [(8, 16), (8, 32), (16, 32), (64, 128)]


def test_params_match_the_fixtures_digest():
    for path in golden_files("toklong_*.npz"):
        d = np.load(path)
        assert str(d["meta.params_sha256"]) == synth.digest(synth.float_params(int(d["meta.seed"]), E=int(d["meta.E"]))), path


@pytest.mark.parametrize("E", [64, 128])
def test_anchor_equals_the_fixed_tokenizer_bit_for_bit(oracle, E):
    """60 x 90 -> 8 x 16 on f32 frames: the composed definition is oracle.tokenizer"""
    img = (synth.frames(3, 2)["img_u8"].astype(np.float32) / np.float32(255.0))
    cw, cb, lw, lb = tok_params(E)
    want = oracle.tokenizer(img, cw.reshape(E, 1, 7, 7), cb, lw, lb)
    np.testing.assert_array_equal(composed(oracle, img, 8, 16, E), want)


def test_fixtures_from_the_reference_within_2e_5(oracle):
    """the reference's own OverlapPatchMerging (tools/gen_tokenizer_long_golden.py); 2e-5 is the project's bound for
    float stages against PyTorch"""
    paths = golden_files("toklong_*.npz")
    assert len(paths) == 6
    for path in paths:
        d = np.load(path)
        E, th, tw = int(d["meta.E"]), int(d["meta.tok_h"]), int(d["meta.tok_w"])
        got = composed(oracle, d["img"], th, tw, E, seed=int(d["meta.seed"]))
        err = float(np.abs(got - d["tokens"]).max())
        print(os.path.basename(path), "max |definition - reference| =", err)
        assert got.shape == d["tokens"].shape and err <= 2e-5, (path, err)


@pytest.mark.parametrize("shape,grid", [((97, 131), (8, 16)), ((20, 30), (8, 32)), ((7, 9), (8, 16)), ((1, 1), (8, 16)),
                                        ((120, 180), (16, 32)), ((8, 4096), (8, 16)), ((4096, 8), (8, 16))])
def test_definition_within_1e_5_of_float64(oracle, shape, grid):
    rs = np.random.RandomState(shape[0] * 4099 + shape[1])
    img = rs.uniform(0, 1, size=(2,) + shape).astype(np.float32)
    for E in (64, 128):
        cw, cb, lw, lb = tok_params(E)
        got = composed(oracle, img, *grid, E)
        want = tl.tokens_f64(img, *grid, cw, cb, lw, lb)
        err = float(np.abs(got - want).max())
        print(shape, grid, E, "max |f32 - f64| =", err)
        assert err <= 1e-5


def test_pixel_values_and_dtypes(oracle):
    """u8 / u16 / i16 frames are valued as ita_ingest values them, before the blend"""
    rs = np.random.RandomState(11)
    u8 = rs.randint(0, 256, size=(1, 33, 47)).astype(np.uint8)
    np.testing.assert_array_equal(tl.blend_patches(u8, 8, 16), tl.blend_patches(u8.astype(np.float32) / np.float32(255.0), 8, 16))
    u16 = rs.randint(0, 65536, size=(1, 33, 47)).astype(np.uint16)
    scale = 1.0 / 40000.0                                  # saturates the codes above 40000
    v = np.minimum(u16.astype(np.float32) * np.float32(scale), np.float32(1.0))
    assert (v == 1.0).any() and (v < 1.0).any()
    np.testing.assert_array_equal(tl.blend_patches(u16, 8, 16, scale), tl.blend_patches(v, 8, 16))
    np.testing.assert_array_equal(tl.blend_patches(u16.view(np.int16), 8, 16, scale), tl.blend_patches(v, 8, 16))


def _check_axis(n_in, n_out, i0, ip, l1):
    assert i0.min() >= 0 and (i0 + ip).max() <= n_in - 1, (n_in, n_out)
    assert l1.dtype == np.float32 and l1.min() >= 0.0 and l1.max() < 1.0, (n_in, n_out)
    # the clamp of the definition is the one at 0 (src = max(scale * (dst + 0.5) - 0.5, 0)): there the source is pixel 0
    # alone, l1 = 0 exactly, whether or not a second neighbour exists (ip = 0 when the grid has one pixel)
    raw = np.float32(n_in) / np.float32(n_out) * (np.arange(n_out, dtype=np.float32) + np.float32(0.5)) - np.float32(0.5)
    assert (l1[raw <= 0] == 0.0).all() and (i0[raw <= 0] == 0).all(), (n_in, n_out)
    # no second neighbour (ip = 0) only on the last pixel of the grid: an up-sampling resize ends with src in
    # (n_in - 1, n_in - 0.5), where PyTorch too keeps l1 > 0 and blends the last pixel with itself
    assert (i0[ip == 0] == n_in - 1).all(), (n_in, n_out)


def test_geometry_sweep():
    """every frame size 1..4096 (the axes are independent: each size is swept as a height and as a width) against every
    token-grid size in use: the neighbours stay on the conv grid, 0 <= l1 < 1, and l1 = 0 at the clamp"""
    outs_h = sorted({g[0] for g in GRIDS} | {1, 4, 128, 512})
    outs_w = sorted({g[1] for g in GRIDS} | {64, 256, 4096})
    for n in range(1, 4097):
        for th in outs_h:
            (y0, yp, ly), _ = tl.geometry(n, 1, th, 16)
            _check_axis((n - 1) // 2 + 1, th, y0, yp, ly)
        for tw in outs_w:
            _, (x0, xp, lx) = tl.geometry(1, n, 1, tw)
            _check_axis((n - 1) // 2 + 1, tw, x0, xp, lx)
    with pytest.raises(ValueError):
        tl.geometry(0, 5, 8, 16)
    with pytest.raises(ValueError):
        tl.geometry(5, 4097, 8, 16)


def test_geometry_matches_the_fixed_tokenizer():
    (y0, yp, ly), (x0, xp, lx) = tl.geometry(60, 90, 8, 16)
    assert y0.tolist() == [1, 5, 8, 12, 16, 20, 23, 27] and yp.tolist() == [1] * 8 and xp.tolist() == [1] * 16
    assert x0.max() == 43 and float(ly[0]) == 0.375 and float(lx[0]) == 0.90625


def test_symbol_declared_listed_and_exported():
    """fails on the commit before the long tokenizer existed"""
    hdr = open(os.path.join(REPO, "include", "ita_mi355x.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    s = r"\s*"
    pat = (r"\bint\s+ita_tokenizer_long\s*\(\s*ita_handle\s+h\s*,\s*const\s+void\s*\*\s*src_dev\s*,\s*int\s+pixel_dtype\s*,\s*int\s+height\s*,"
           r"\s*int\s+width\s*,\s*long\s+long\s+row_stride\s*,\s*long\s+long\s+frame_stride\s*,\s*float\s+depth_scale\s*,\s*int\s+tok_h\s*,"
           r"\s*int\s+tok_w\s*,\s*float\s*\*\s*tokens_dev\s*,\s*int\s+batch\s*,\s*void\s*\*\s*stream\s*\)" + s + ";")
    assert re.search(pat, hdr)
    assert "ita_tokenizer_long" in host.EXPORTED_SYMBOLS
    lib = ctypes.CDLL(host.build_extension())
    assert hasattr(lib, "ita_tokenizer_long")
    assert lib.ita_abi_version() == 1


def test_python_signatures():
    sig = inspect.signature(host.Engine.tokenize_long)
    assert list(sig.parameters) == ["self", "frames", "tok_h", "tok_w", "depth_scale", "out"]
    assert sig.parameters["depth_scale"].default is None and sig.parameters["out"].default is None
    sig = inspect.signature(host.Engine.encode_frames_long)
    assert list(sig.parameters) == ["self", "frames", "tok_h", "tok_w", "depth_scale"]
    assert sig.parameters["depth_scale"].default is None


def test_definition_does_not_load_the_oracle():
    src = open(os.path.join(REPO, "drone-oa-iree-vit-accelerator_amd", "tokenizer_long_ref.py")).read()
    assert not re.search(r"^\s*(from|import)\s+\.*oracle", src, flags=re.M)
