"""CPU-side checks of the ingest stage (refine_inputs' resize of camera-resolution frames): the numpy definition
ingest_ref.ingest_reference against torch's CPU F.interpolate, its pixel-value rules, and the ita_ingest entry's export
and argument checks (which run before the entry touches its handle or the GPU).  No compute call is made here."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from conftest import REPO
from drone_oa_iree_vit_accelerator_amd import host, ingest_ref, replay
from drone_oa_iree_vit_accelerator_amd.ingest_ref import ingest_reference

EXACT_SIZES = [(120, 180), (480, 720)]                      # every weight is exactly 0.5
CLOSE_SIZES = [(480, 640), (270, 480), (240, 320), (720, 1280), (480, 848), (64, 96), (75, 100), (61, 91), (59, 89)]
TORCH_BOUND = 5e-6    # torch rounds its weights differently; measured <= 1.8e-6 on these sizes, about 3 x margin


def _torch_resize(values):
    import torch
    import torch.nn.functional as F
    t = torch.from_numpy(values)[:, None]
    return F.interpolate(t, size=(60, 90), mode="bilinear", align_corners=False)[:, 0].numpy()


def _u8_frames(H, W):
    return np.random.RandomState(0).randint(0, 256, size=(3, H, W)).astype(np.uint8)


@pytest.mark.parametrize("H,W", EXACT_SIZES)
def test_reference_equals_torch_where_weights_are_exact(H, W):
    raw = _u8_frames(H, W)
    got = ingest_reference(raw)
    assert got.shape == (3, 60, 90) and got.dtype == np.float32
    np.testing.assert_array_equal(got, _torch_resize(raw.astype(np.float32) / np.float32(255)))


@pytest.mark.parametrize("H,W", CLOSE_SIZES)
def test_reference_close_to_torch(H, W):
    raw = _u8_frames(H, W)
    err = float(np.abs(ingest_reference(raw) - _torch_resize(raw.astype(np.float32) / np.float32(255))).max())
    print(f"{H}x{W}: max |ingest_reference - torch| = {err:.3e}")
    assert err <= TORCH_BOUND


def test_u16_depth_scale_and_clip():
    rs = np.random.RandomState(0)
    raw = rs.randint(0, 20000, size=(3, 240, 320)).astype(np.uint16)
    assert (raw > 10000).any() and (raw < 10000).any()
    v = ingest_ref.pixel_values(raw, 1e-4)
    assert v.dtype == np.float32 and float(v.max()) == 1.0
    assert (v[raw > 10000] == 1.0).all()                                   # 10001 * 1e-4 already exceeds 1
    lo = raw <= 10000
    np.testing.assert_allclose(v[lo], raw[lo].astype(np.float64) * 1e-4, rtol=3e-7, atol=0)   # two f32 roundings
    got = ingest_reference(raw, depth_scale=1e-4)
    assert float(got.max()) <= 1.0
    err = float(np.abs(got - _torch_resize(v)).max())
    print(f"u16 240x320: max |ingest_reference - torch| = {err:.3e}")
    assert err <= TORCH_BOUND
    # a frame wholly behind the clip is 1.0 everywhere: the weights of a pair sum to exactly 1
    np.testing.assert_array_equal(ingest_reference(np.full((1, 240, 320), 20000, np.uint16), 1e-4), np.ones((1, 60, 90), np.float32))
    # int16 is taken as the same bits
    np.testing.assert_array_equal(ingest_reference(raw.view(np.int16), 1e-4), got)
    # the default scale maps the full code range onto [0, 1]
    assert float(ingest_ref.pixel_values(np.array([[65535]], np.uint16)).max()) == 1.0


def test_f32_at_60x90_is_the_identity():
    x = np.random.RandomState(1).standard_normal((2, 60, 90)).astype(np.float32)
    np.testing.assert_array_equal(ingest_reference(x), x)


def test_reference_rejects_what_the_entry_rejects():
    with pytest.raises(ValueError):
        ingest_reference(np.zeros((1, 4097, 8), np.uint8))
    with pytest.raises(ValueError):
        ingest_reference(np.zeros((7,), np.uint8))
    with pytest.raises(TypeError):
        ingest_reference(np.zeros((1, 8, 8), np.float64))


@pytest.fixture(scope="module")
def so():
    return host.build_extension()


def test_symbol_declared_listed_and_exported(so):
    hdr = open(os.path.join(REPO, "include", "ita_mi355x.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+ita_ingest\s*\(", hdr)
    assert re.search(r"ITA_PIXEL_U8\s*=\s*0\s*,\s*ITA_PIXEL_U16\s*=\s*1\s*,\s*ITA_PIXEL_F32\s*=\s*2", hdr)
    assert "ita_ingest" in host.EXPORTED_SYMBOLS
    lib = ctypes.CDLL(so)
    assert hasattr(lib, "ita_ingest")
    assert lib.ita_abi_version() == 1
    assert (host.PIXEL_U8, host.PIXEL_U16, host.PIXEL_F32) == (0, 1, 2)
    assert "ita_ingest" in open(os.path.join(REPO, "INTEGRATION.md")).read()


def test_blend_and_coordinates_are_compiled_with_contraction_off():
    """the no-fma property holds by construction in the kernel source, not through a build flag: each of the three
    functions with a multiply feeding an add or a subtract carries the pragma"""
    src = open(os.path.join(REPO, "drone-oa-iree-vit-accelerator_amd", "csrc", "ita_ingest_kernel.h")).read()
    for fn in ("ItaIngestCoord ita_ingest_coord(", "float ita_ingest_px(uint16_t", "float ita_ingest_blend("):
        body = src[src.index(fn):]
        body = body[:body.index("\n}\n")]
        assert "#pragma clang fp contract(off)" in body, fn


def test_python_signatures():
    sig = inspect.signature(host.Engine.ingest)
    assert list(sig.parameters) == ["self", "frames", "depth_scale", "out"]
    assert sig.parameters["depth_scale"].default is None and sig.parameters["out"].default is None
    rs = inspect.signature(replay.replay_frames)
    assert list(rs.parameters) == ["engine", "root", "max_batch", "schedule", "resize"]
    assert rs.parameters["resize"].default == "pil"
    assert rs.parameters["schedule"].default == "steps" and rs.parameters["max_batch"].default == 1024
    assert "resize" not in inspect.signature(replay.replay).parameters      # replay() keeps its signature: the host resize


def test_replay_rejects_unknown_resize_before_touching_the_engine(tmp_path):
    class NoEngine:
        def __getattr__(self, name):
            raise AssertionError(f"the engine was touched ({name}) before resize was checked")
    with pytest.raises(ValueError):
        replay.replay_frames(NoEngine(), str(tmp_path / "missing"), resize="stb")


def test_entry_refuses_bad_arguments_without_a_gpu(so):
    """ita_ingest judges every argument before it uses its handle or makes a HIP call, so the refusals can be exercised
    here: a null handle, and -- behind a non-null stand-in handle that is never dereferenced -- each rule of the header.
    (A call with VALID arguments is not made: it would go on to the GPU.)"""
    L = host.lib()
    INVALID = -1
    fake_handle = ctypes.create_string_buffer(1 << 16)     # zeroed and large: never read by a refused call
    src = ctypes.create_string_buffer(64)
    dst = ctypes.create_string_buffer(64)
    h, s, d = ctypes.addressof(fake_handle), ctypes.addressof(src), ctypes.addressof(dst)
    assert s % 4 == 0 and d % 4 == 0
    good = dict(h=h, src=s, dt=host.PIXEL_U16, H=480, W=640, rs=640, fs=480 * 640, scale=1e-4, dst=d, batch=2)

    def call(**kw):
        a = dict(good, **kw)
        return L.ita_ingest(a["h"], a["src"], a["dt"], a["H"], a["W"], a["rs"], a["fs"], a["scale"], a["dst"], a["batch"], None)

    bad = [dict(h=None), dict(src=None), dict(dst=None), dict(dt=3), dict(dt=-1), dict(H=0), dict(H=4097), dict(W=0),
           dict(W=4097), dict(rs=639), dict(fs=479 * 640 + 639), dict(batch=0), dict(batch=-3), dict(scale=0.0),
           dict(scale=-1e-4), dict(scale=float("inf")), dict(scale=float("nan")), dict(src=s + 1)]
    for kw in bad:
        assert call(**kw) == INVALID, kw
        assert L.ita_last_error() == INVALID and L.ita_error_string()
