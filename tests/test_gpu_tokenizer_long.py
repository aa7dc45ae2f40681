"""The long-sequence tokenizer on the MI355X (ita_tokenizer_long / Engine.tokenize_long / encode_frames_long): bit for bit
against the definition composed in tests/test_tokenizer_long_cpu.py (tokenizer_long_ref.blend_patches, then the oracle's
fmaf chain and LayerNorm), and at 60 x 90 -> 8 x 16 against the fixed tokenizer (Engine.tokenizer).

Blobs: vitlstm_E64_seed0_B2 (E = 64, one layer) and vit2l_E128_s0_B2 (E = 128, int8, two layers)."""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import golden_files
from drone_oa_iree_vit_accelerator_amd import host, params, synth
from drone_oa_iree_vit_accelerator_amd import tokenizer_long_ref as tl
from gpu_support import cu, engine_pool
from tokenizer_long_common import composed, tok_params

pytestmark = pytest.mark.gpu

CANARY = -12345.0
INVALID_ARG, UNSUPPORTED = -1, -4
# frame, grid: the whole table runs at E = 64 and E = 128, two frames each.  The kernel's form by the horizontal ratio CW / tok_w:
# LDS window at 20 x 30 (0.47), 7 x 9 (0.31), 1 x 1, 120 x 180 (2.8), 4096 x 8 (0.25); direct loads at 97 x 131 (4.1), 8 x 4096 (128)
SHAPES = [((97, 131), (8, 16)), ((20, 30), (8, 32)), ((7, 9), (8, 16)), ((1, 1), (8, 16)), ((120, 180), (16, 32)),
          ((8, 4096), (8, 16)), ((4096, 8), (8, 16)),
          # the threshold between the two forms at a 16-token row: conv width 63 (a tile spans 127 columns, window) and 64 (129, direct)
          ((9, 126), (8, 16)), ((9, 127), (8, 16))]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@functools.lru_cache(maxsize=None)
def _blob(E):
    if E == 64:
        d, fp, nl = params.load_fixture(golden_files("vitlstm_E64_seed0_B2.npz")[0]), synth.float_params(0, E=64), 1
    else:
        d, nl = params.load_fixture(golden_files("vit2l_E128_s0_B2.npz")[0]), 2
        fp = synth.float_params(0, E=128, num_layers=2, tail=False)
    # the composed definition takes its parameters from tok_params(E): the blob's tokenizer must hold the same
    for got, want in zip(tok_params(E), ("tokenizer.conv.weight", "tokenizer.conv.bias", "tokenizer.norm.weight", "tokenizer.norm.bias")):
        np.testing.assert_array_equal(got.reshape(-1), fp[want].reshape(-1))
    return params.blob_from_record(d, fp, E=E, num_layers=nl)


@pytest.fixture(scope="module")
def engines(torch_cuda):
    yield from engine_pool(_blob)


def _frames(dtype, shape, seed):
    rs = np.random.RandomState(seed)
    if dtype == "u8":
        return rs.randint(0, 256, size=shape).astype(np.uint8)
    if dtype in ("u16", "i16"):
        a = rs.randint(0, 65536, size=shape).astype(np.uint16)
        return a.view(np.int16) if dtype == "i16" else a
    return rs.uniform(0, 1, size=shape).astype(np.float32)


def _guarded(torch, eng, frames, th, tw, n, depth_scale=None):
    """Engine.tokenize_long into a canary-filled buffer with 64 canary floats directly behind the tokens -> numpy"""
    size = n * th * tw * eng.E
    buf = torch.full((size + 64,), CANARY, dtype=torch.float32, device="cuda")
    out = buf[:size].view(n, th * tw, eng.E)
    got = eng.tokenize_long(frames, th, tw, depth_scale=depth_scale, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    hb = buf.cpu().numpy()
    assert (hb[size:] == CANARY).all(), "floats behind tokens_dev were written"
    return hb[:size].reshape(n, th * tw, eng.E)


def _same_bits(got, want):
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape
    diff = got.view(np.uint32) != want.view(np.uint32)
    assert not diff.any(), f"{int(diff.sum())} of {diff.size} values differ, max |diff| = {float(np.abs(got - want).max()):.3e}"


# ---- anchor: the fixed tokenizer
@pytest.mark.parametrize("B", [1, 3, 300])
@pytest.mark.parametrize("E", [64, 128])
def test_anchor_equals_the_fixed_tokenizer(torch_cuda, engines, E, B):
    """60 x 90 -> 8 x 16: f32 frames give Engine.tokenizer's bits on the same frames; u8 frames give those of the frames
    divided by 255 (f32(code) / 255.0f, correctly rounded: divided on the host) -- not those of the u8 wire form, which
    folds the division into the conv weights and agrees to ~1e-6 only.  300 frames: more than there are CUs."""
    torch, eng = torch_cuda, engines(E)
    u8 = _frames("u8", (B, 60, 90), 100 + B)
    f32 = cu(u8.astype(np.float32) / np.float32(255.0))
    want = eng.tokenizer(f32)
    assert torch.equal(eng.tokenize_long(f32, 8, 16), want)
    assert torch.equal(eng.tokenize_long(cu(u8), 8, 16), want)
    wire = eng.tokenizer(cu(u8))
    assert float((wire - want).abs().max()) <= 2e-5


# ---- shapes: the composed definition
@pytest.mark.parametrize("shape,grid", SHAPES, ids=[f"{s[0]}x{s[1]}-T{g[0]}x{g[1]}" for s, g in SHAPES])
@pytest.mark.parametrize("E", [64, 128])
def test_shapes_equal_the_definition(torch_cuda, engines, oracle, E, shape, grid):
    f = _frames("f32", (2,) + shape, shape[0] * 4099 + shape[1])
    _same_bits(_guarded(torch_cuda, engines(E), cu(f), *grid, 2), composed(oracle, f, *grid, E))


def test_config5_shape(torch_cuda, engines, oracle):
    """480 x 720 -> 64 x 128 = 8192 tokens, E = 128, u8 frames"""
    f = _frames("u8", (2, 480, 720), 5)
    _same_bits(_guarded(torch_cuda, engines(128), cu(f), 64, 128, 2), composed(oracle, f, 64, 128, 128))


@pytest.mark.parametrize("shape", [(97, 131), (61, 93)], ids=["97x131-direct", "61x93-window"])
@pytest.mark.parametrize("dtype", ["u8", "u16", "i16", "f32"])
@pytest.mark.parametrize("E", [64, 128])
def test_every_dtype(torch_cuda, engines, oracle, E, dtype, shape):
    """-> 8 x 16.  97 x 131: horizontal ratio 4.1, the direct-load form; 61 x 93: 2.9, the LDS-window form.  The 16-bit
    depth_scale saturates the codes above 40000"""
    f = _frames(dtype, (2,) + shape, 17)
    scale = 1.0 / 40000.0 if dtype in ("u16", "i16") else None
    if scale:
        v = tl.pixel_values(f, scale)
        assert (v == 1.0).any() and (v < 1.0).any()
    _same_bits(_guarded(torch_cuda, engines(E), cu(f), 8, 16, 2, depth_scale=scale), composed(oracle, f, 8, 16, E, scale))


def test_inf_where_only_a_pad_slot_could_reach(torch_cuda, engines, oracle):
    """The K = 52 chain has three pad slots behind tap 48 = (ky 6, kx 6).  A kernel that let them carry 'tap 49..51' =
    (ky 7, kx 0..2) times a zero weight would read row 2 y0 + 4 [+ 2] of a token; at 97 x 131 -> 8 x 16 the patches of
    neighbouring token rows leave rows between them that no real tap reads.  An inf there must not reach any token."""
    H, W, th, tw = 97, 131, 8, 16
    (y0, yp, _), (x0, xp, _) = tl.geometry(H, W, th, tw)
    rows = set()
    for a, p in zip(y0.tolist(), yp.tolist()):
        rows |= set(range(2 * a - 3, 2 * a + 4)) | set(range(2 * a - 3 + 2 * p, 2 * a + 4 + 2 * p))
    oy = 2
    bad_row = 2 * int(y0[oy]) + 4 + 2 * int(yp[oy])           # ky = 7 of the second neighbour row
    assert 0 <= bad_row < H and bad_row not in rows
    f = _frames("f32", (2, H, W), 23)
    f[:, bad_row, :] = np.inf
    want = composed(oracle, f, th, tw, 64)
    assert np.isfinite(want).all()
    for E in (64, 128):
        got = _guarded(torch_cuda, engines(E), cu(f), th, tw, 2)
        assert np.isfinite(got).all()
        _same_bits(got, composed(oracle, f, th, tw, E))


# ---- views
@pytest.mark.parametrize("dtype", ["u8", "u16", "f32"])
def test_cropped_misaligned_view_is_read_through_its_strides(torch_cuda, engines, oracle, dtype):
    """a crop of a larger buffer whose first pixel lies one pixel behind an aligned address: no copy is made (the view's
    own strides reach the C entry) and the tokens are those of the contiguous copy"""
    torch, eng = torch_cuda, engines(64)
    big = _frames(dtype, (3, 140, 201), 31)
    view = cu(big)[:, 7:7 + 97, 34:34 + 131]
    px = view.element_size()
    assert not view.is_contiguous() and (view.data_ptr() // px) % 2 == 1
    assert eng._frame_strides(view) == (201, 140 * 201)
    got = _guarded(torch, eng, view, 8, 16, 3)
    _same_bits(got, eng.tokenize_long(cu(big[:, 7:7 + 97, 34:34 + 131]), 8, 16).cpu().numpy())
    _same_bits(got, composed(oracle, big[:, 7:7 + 97, 34:34 + 131], 8, 16, 64))


# ---- determinism, batch independence, streams
@pytest.mark.parametrize("E", [64, 128])
def test_frames_do_not_depend_on_their_batch_or_stream(torch_cuda, engines, E):
    torch, eng = torch_cuda, engines(E)
    f = cu(_frames("u8", (5, 120, 180), 41))
    a = eng.tokenize_long(f, 16, 32)
    assert torch.equal(a, eng.tokenize_long(f, 16, 32))
    assert torch.equal(eng.tokenize_long(f[3:4], 16, 32), a[3:4])
    assert torch.equal(eng.tokenize_long(f.flip(0).contiguous(), 16, 32).flip(0), a)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        b = eng.tokenize_long(f, 16, 32)
    s.synchronize()
    assert torch.equal(a, b)


# ---- the chain
def test_encode_frames_long_is_tokenize_then_encode(torch_cuda, engines):
    """the int8 E = 128 two-layer blob: encode_frames_long = encode_long(tokenize_long), and ita_fusion_tail_large takes it"""
    torch, eng = torch_cuda, engines(128)
    assert eng.num_layers == 2 and eng.attn_kind(0) == host.ATTN_INT8 and eng.ffn_kind(0) == host.FFN_INT8
    f = cu(_frames("u8", (2, 120, 180), 43))
    got = eng.encode_frames_long(f, 16, 32)
    assert tuple(got.shape) == (2, 512, 128)
    assert torch.equal(got, eng.encode_long(eng.tokenize_long(f, 16, 32)))
    c = synth.tail_large_case(0, 128, 16, 32, 48, 1)
    tail = host.FusionTailLarge(c["conv_w"], c["conv_b"], device=0)
    fmap = tail(got, 16, 32)
    torch.cuda.synchronize()
    assert tuple(fmap.shape) == (2, 48, 32, 64) and bool(torch.isfinite(fmap).all()) and float(fmap.std()) > 0
    tail.close()


# ---- refusals
def _call(eng, src, dtype, H, W, rs, fs, scale, th, tw, out, batch):
    return host.lib().ita_tokenizer_long(eng._h, src, dtype, H, W, rs, fs, C.c_float(scale), th, tw, out, batch,
                                         host._stream_ptr(eng.device))


def test_refusals_before_any_launch(torch_cuda, engines, oracle):
    """every INVALID_ARG and UNSUPPORTED case of the entry returns its status and leaves a canary-filled output as it
    was; the handle then runs normally"""
    torch, eng = torch_cuda, engines(64)
    H, W, th, tw = 20, 30, 8, 16
    f = _frames("u8", (2, H, W), 47)
    src = cu(f)
    out = torch.full((2 * 1024 * 64,), CANARY, dtype=torch.float32, device="cuda")   # room for 2 x 1024 tokens of E = 64
    s, o, ds = src.data_ptr(), out.data_ptr(), 1.0 / 65535.0
    ok = dict(src=s, dtype=host.PIXEL_U8, H=H, W=W, rs=W, fs=H * W, scale=ds, th=th, tw=tw, out=o, batch=2)
    invalid = [dict(src=None), dict(out=None), dict(dtype=3), dict(dtype=-1), dict(H=0), dict(H=4097), dict(W=0), dict(W=4097),
               dict(rs=W - 1), dict(fs=H * W - 1), dict(rs=(1 << 40) + 1, fs=(1 << 41)), dict(fs=(1 << 40) + 1), dict(batch=0),
               dict(batch=-1), dict(dtype=host.PIXEL_U16, src=s + 1), dict(dtype=host.PIXEL_F32, src=s + 2), dict(out=o + 4),
               dict(dtype=host.PIXEL_U16, scale=0.0), dict(dtype=host.PIXEL_U16, scale=-1.0),
               dict(dtype=host.PIXEL_U16, scale=float("inf")), dict(dtype=host.PIXEL_U16, scale=float("nan"))]
    unsupported = [dict(tw=24), dict(tw=8, th=16), dict(tw=0), dict(tw=-16), dict(th=0), dict(th=-8), dict(th=4, tw=16),
                   dict(th=9, tw=16), dict(th=1024, tw=80), dict(batch=65536)]
    for status, cases in ((INVALID_ARG, invalid), (UNSUPPORTED, unsupported)):
        for c in cases:
            assert _call(eng, **{**ok, **c}) == status, c
    assert host.lib().ita_tokenizer_long(None, s, host.PIXEL_U8, H, W, W, H * W, C.c_float(ds), th, tw, o, 2, None) == INVALID_ARG
    torch.cuda.synchronize()
    assert bool((out == CANARY).all()), "a refused call wrote to its output"
    with pytest.raises(host.ITAError, match="ita status -4"):
        eng.tokenize_long(src, 8, 24)
    with pytest.raises(host.ITAError):
        eng.tokenize_long(src, 8, 16, out=torch.empty((2, 128, 32), device="cuda"))
    with pytest.raises(host.ITAError):
        eng.tokenize_long(src.cpu(), 8, 16)
    assert _call(eng, **ok) == 0
    torch.cuda.synchronize()
    _same_bits(out[:2 * 128 * 64].cpu().numpy().reshape(2, 128, 64), composed(oracle, f, th, tw, 64))
    assert bool((out[2 * 128 * 64:] == CANARY).all())


def test_a_handle_without_weights_is_refused(torch_cuda):
    """ITA_ERR_NO_WEIGHTS (-3), the status the other compute entries give for it"""
    torch = torch_cuda
    h = C.c_void_p()
    host._chk(host.lib().ita_create(C.byref(h), 0))
    src = torch.zeros((1, 20, 30), dtype=torch.uint8, device="cuda")
    out = torch.full((128 * 64,), CANARY, dtype=torch.float32, device="cuda")
    assert host.lib().ita_tokenizer_long(h, src.data_ptr(), host.PIXEL_U8, 20, 30, 30, 600, C.c_float(1.0), 8, 16, out.data_ptr(), 1, None) == -3
    assert host.lib().ita_tokenizer(h, src.data_ptr(), host.IMAGE_U8, out.data_ptr(), 1, None) == -3
    torch.cuda.synchronize()
    assert bool((out == CANARY).all())
    host.lib().ita_destroy(h)


# ---- profiling
def test_profiling_counts_a_call_as_the_tokenizer_stage(torch_cuda, engines):
    """between profile_begin(only_stage="tokenizer") and profile_end every sampled call is one forward with a tokenizer time
    and nothing else; with all stages selected the call, which is no whole forward, is not counted; the tokens do not change"""
    torch, eng = torch_cuda, engines(64)
    f = cu(_frames("u8", (2, 120, 180), 53))
    want = eng.tokenize_long(f, 16, 32)
    eng.profile_begin(8, every_n=2, only_stage="tokenizer")
    got = [eng.tokenize_long(f, 16, 32) for _ in range(4)]
    ms, n = eng.profile_end()
    assert n == 2 and ms["tokenizer"] > 0 and all(v == 0 for k, v in ms.items() if k != "tokenizer")
    eng.profile_begin(4)
    got.append(eng.tokenize_long(f, 16, 32))
    ms, n = eng.profile_end()
    assert n == 0 and all(v == 0 for v in ms.values())
    assert all(torch.equal(g, want) for g in got)
