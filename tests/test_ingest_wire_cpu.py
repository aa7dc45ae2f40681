"""CPU-side checks of the wire ingest (the reference host's stb resize of camera frames to u8 wire frames): the numpy
definition ingest_wire_ref.ingest_wire_reference against stb's own output (tests/golden/resize_stb_*.npz, written by
tools/gen_resize_golden.py from the reference's vendored header), the C++ table builder ita_resize_table against the
definition's tables bit for bit, and the entry's exports and argument checks.  No compute call is made here."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from conftest import REPO, golden_files
from drone_oa_iree_vit_accelerator_amd import host, ingest_wire_ref, replay
from drone_oa_iree_vit_accelerator_amd.ingest_wire_ref import ingest_wire_reference, resize_tables

SIZES = ["96x128", "480x640", "720x1280", "61x93", "30x45", "100x64", "1x200", "200x1", "1x1", "8x4096", "4096x8"]
ONE_PIXEL_AXIS = {"1x200", "200x1", "1x1"}     # one tie fills a whole row or column there: no count gate
TIE = 1e-3                                     # |v - round(v)| of a code that differs from stb's
MAX_DIFFERING = 27                             # 0.5 % of a frame's 5400 codes


@pytest.mark.parametrize("size", SIZES)
def test_definition_against_stb(size):
    d = np.load(golden_files(f"resize_stb_{size}.npz")[0])
    src, stb = d["src"], d["stb"]
    assert src.shape[0] == 5 and src.shape[1:] == tuple(int(v) for v in size.split("x")) and stb.shape == (5, 60, 90)
    codes, v = ingest_wire_reference(src, return_values=True)
    assert codes.dtype == np.uint8 and codes.shape == stb.shape and v.dtype == np.float32
    diff = codes.astype(np.int32) - stb.astype(np.int32)
    differs = diff != 0
    per_frame = differs.reshape(5, -1).sum(axis=1)
    tie = float(np.abs(v - np.rint(v))[differs].max()) if differs.any() else 0.0
    print(f"{size}: max |code - stb| = {int(np.abs(diff).max())}, differing codes per frame = {per_frame.tolist()}, "
          f"largest |v - round(v)| among them = {tie:.3e}")
    assert int(np.abs(diff).max()) <= 1
    assert tie <= TIE
    if size not in ONE_PIXEL_AXIS:
        assert int(per_frame.max()) <= MAX_DIFFERING


TABLE_PAIRS = [(480, 60), (640, 90), (720, 60), (1280, 90), (61, 60), (93, 90), (30, 60), (45, 90), (1, 60), (4096, 90),
               (60, 60), (90, 90)]


@pytest.mark.parametrize("n_in,n_out", TABLE_PAIRS)
def test_cpp_table_equals_definition_bit_for_bit(n_in, n_out):
    host.build_extension()
    n0, count, coeff = resize_tables(n_in, n_out)
    g0, gcount, gcoeff = host.resize_table(n_in, n_out)
    assert n0.dtype == np.int32 and count.dtype == np.int32 and coeff.dtype == np.float32
    np.testing.assert_array_equal(g0, n0)
    np.testing.assert_array_equal(gcount, count)
    assert gcoeff.shape == coeff.shape and coeff.shape[1] == int(count.max())
    assert (gcoeff.view(np.uint32) == coeff.view(np.uint32)).all()
    # what the kernel relies on: every tap inside the source, the padding zero, every row sums to 1 within rounding
    assert (n0 >= 0).all() and (count >= 1).all() and (n0 + count <= n_in).all()
    for o in range(n_out):
        assert not coeff[o, count[o]:].any()
    np.testing.assert_allclose(coeff.astype(np.float64).sum(axis=1), 1.0, atol=1e-6, rtol=0)


def test_table_entry_reports_width_and_refuses_bad_arguments():
    host.build_extension()
    L = host.lib()
    n0, count = np.zeros(90, np.int32), np.zeros(90, np.int32)
    coeff = np.zeros((90, 64), np.float32)
    width = ctypes.c_int(0)
    args = (n0.ctypes.data, count.ctypes.data, coeff.ctypes.data)
    assert L.ita_resize_table(640, 90, *args, 64, ctypes.byref(width)) == 0 and width.value == 29
    np.testing.assert_array_equal(coeff[:, :29], resize_tables(640, 90)[2])
    assert not coeff[:, 29:].any()
    assert L.ita_resize_table(640, 90, *args, 28, ctypes.byref(width)) == -1 and width.value == 29   # too narrow
    for n_in, n_out in ((0, 90), (4097, 90), (640, 0)):
        assert L.ita_resize_table(n_in, n_out, *args, 64, ctypes.byref(width)) == -1
    assert L.ita_resize_table(640, 90, None, count.ctypes.data, coeff.ctypes.data, 64, ctypes.byref(width)) == -1


def test_a_60x90_source_comes_out_unchanged():
    raw = np.random.RandomState(3).randint(0, 256, size=(3, 60, 90)).astype(np.uint8)
    raw[0, 0, :2] = (0, 255)
    np.testing.assert_array_equal(ingest_wire_reference(raw), raw)
    for n in (60, 90):
        n0, count, coeff = resize_tables(n, n)
        np.testing.assert_array_equal(n0, np.arange(n))
        assert (count == 1).all() and (coeff == 1.0).all()


def test_leading_dimensions_collapse_and_bad_input_is_refused():
    raw = np.random.RandomState(4).randint(0, 256, size=(2, 2, 75, 100)).astype(np.uint8)
    got = ingest_wire_reference(raw)
    assert got.shape == (4, 60, 90)
    np.testing.assert_array_equal(got[3], ingest_wire_reference(raw[1, 1])[0])
    with pytest.raises(TypeError):
        ingest_wire_reference(raw.astype(np.uint16))
    with pytest.raises(ValueError):
        ingest_wire_reference(np.zeros((1, 4097, 8), np.uint8))
    with pytest.raises(ValueError):
        ingest_wire_reference(np.zeros((7,), np.uint8))


def test_definition_needs_no_torch():
    src = open(ingest_wire_ref.__file__).read()
    assert not re.search(r"^\s*(import|from)\s+torch", src, flags=re.M)


def test_symbols_declared_listed_and_exported():
    so = host.build_extension()
    hdr = open(os.path.join(REPO, "include", "ita_mi355x.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = ctypes.CDLL(so)
    for sym in ("ita_ingest_wire", "ita_ingest_wire_prepare", "ita_resize_table"):
        assert re.search(r"\bint\s+" + sym + r"\s*\(", hdr), sym
        assert sym in host.EXPORTED_SYMBOLS and hasattr(lib, sym), sym
    assert "ita_ingest_wire" in open(os.path.join(REPO, "INTEGRATION.md")).read()


def test_kernel_arithmetic_is_compiled_with_contraction_off():
    src = open(os.path.join(REPO, "drone-oa-iree-vit-accelerator_amd", "csrc", "ita_ingest_wire_kernel.h")).read()
    for fn in ("float ita_wire_px(", "void ita_ingest_wire_kernel(", "bool ita_resize_axis(", "float ita_resize_mitchell(",
               "float ita_resize_catmull_rom("):
        body = src[src.index(fn):]
        body = body[:body.index("\n}\n")]
        assert "#pragma clang fp contract(off)" in body, fn


def test_python_signatures_and_replay_modes():
    sig = inspect.signature(host.Engine.ingest_wire)
    assert list(sig.parameters) == ["self", "frames", "out"] and sig.parameters["out"].default is None
    assert list(inspect.signature(host.Engine.prepare_ingest_wire).parameters) == ["self", "H", "W"]
    assert replay.RESIZES == ("pil", "gpu", "stb")
    assert inspect.signature(replay.replay_frames).parameters["resize"].default == "pil"


def test_entry_refuses_bad_arguments_without_a_gpu():
    """ita_ingest_wire judges every argument before it uses its handle or makes a HIP call: a null handle, and -- behind a
    non-null stand-in handle that is never dereferenced -- each rule of the header.  (A call with VALID arguments is not
    made: it would go on to the GPU.)"""
    host.build_extension()
    L = host.lib()
    INVALID = -1
    fake_handle = ctypes.create_string_buffer(1 << 16)
    src, dst = ctypes.create_string_buffer(64), ctypes.create_string_buffer(64)
    good = dict(h=ctypes.addressof(fake_handle), src=ctypes.addressof(src), H=480, W=640, rs=640, fs=480 * 640,
                dst=ctypes.addressof(dst), batch=2)

    def call(**kw):
        a = dict(good, **kw)
        return L.ita_ingest_wire(a["h"], a["src"], a["H"], a["W"], a["rs"], a["fs"], a["dst"], a["batch"], None)

    bad = [dict(h=None), dict(src=None), dict(dst=None), dict(H=0), dict(H=4097), dict(W=0), dict(W=4097), dict(rs=639),
           dict(fs=479 * 640 + 639), dict(rs=(1 << 40) + 4, fs=1 << 62), dict(fs=(1 << 40) + 1), dict(batch=0), dict(batch=-3)]
    for kw in bad:
        assert call(**kw) == INVALID, kw
        assert L.ita_last_error() == INVALID and L.ita_error_string()
    for H, W in ((0, 640), (480, 4097)):
        assert L.ita_ingest_wire_prepare(good["h"], H, W) == INVALID
    assert L.ita_ingest_wire_prepare(None, 480, 640) == INVALID
