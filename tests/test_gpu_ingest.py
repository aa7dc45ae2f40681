"""The ingest kernel (ita_ingest / Engine.ingest) against its definition, ingest_ref.ingest_reference: bit for bit, for
every dtype, size class and stride form the entry accepts, with a guard row of a sentinel in front of and behind the
(N,60,90) output.  Then end to end: ingested frames through forward / forward_sequence."""
import os

import numpy as np
import pytest

from conftest import golden_files
from drone_oa_iree_vit_accelerator_amd import host, params, synth
from drone_oa_iree_vit_accelerator_amd.ingest_ref import ingest_reference

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def fixture_record():
    return params.load_fixture(golden_files("vitlstm_E64_seed0_B2.npz")[0])


@pytest.fixture(scope="module")
def engine(torch_cuda, fixture_record):
    blob = params.blob_from_record(fixture_record, synth.float_params(0, E=64), E=64)
    eng = host.Engine(blob, device=0)
    eng.blob = blob
    yield eng
    eng.close()


def _raw(dtype, shape, seed):
    rs = np.random.RandomState(seed)
    if dtype == "u8":
        return rs.randint(0, 256, size=shape).astype(np.uint8)
    if dtype == "u16":
        return rs.randint(0, 65536, size=shape).astype(np.uint16)
    return rs.uniform(0, 1, size=shape).astype(np.float32)


def _guarded_ingest(torch, eng, frames, n, depth_scale=None):
    """Engine.ingest into the middle of a sentinel-filled buffer with one guard row of 90 floats on each side -> numpy"""
    buf = torch.full((n * 60 + 2, 90), SENTINEL, dtype=torch.float32, device="cuda")
    out = buf[1:-1].view(n, 60, 90)
    got = eng.ingest(frames, depth_scale=depth_scale, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    host_buf = buf.cpu().numpy()
    assert (host_buf[0] == SENTINEL).all() and (host_buf[-1] == SENTINEL).all(), "a guard row was written"
    return host_buf[1:-1].reshape(n, 60, 90)


def _same_bits(got, want):
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape
    diff = got.view(np.uint32) != want.view(np.uint32)
    assert not diff.any(), f"{int(diff.sum())} of {diff.size} outputs differ, max |diff| = {float(np.abs(got - want).max()):.3e}"


# dtype, H, W, batch, depth_scale: the issue's table, then shapes at which the kernels take another path
CASES = [
    ("u8", 480, 640, 3, None),      # scale 8 / 7.11, row skipping (staged rows)
    ("u8", 75, 100, 2, None),       # rows not 16-byte aligned, odd scale (gather)
    ("u8", 61, 91, 1, None),        # scale ~ 1: edge clamps
    ("u8", 59, 89, 1, None),        # upsampling: real < 0, i1 = n - 1
    ("u8", 1, 1, 1, None),          # degenerate axes
    ("u8", 1, 200, 1, None),        # one row, staged (tail of 8 bytes)
    ("u8", 200, 1, 1, None),
    ("u16", 240, 320, 2, 1e-4),     # 2-byte pixels, clip (codes above 10000)
    ("f32", 120, 180, 2, None),     # exact 0.5 weights
    ("u8", 61, 4096, 1, None),      # the widest staged row: 256 16-byte pieces, four per lane
    ("u16", 61, 2049, 1, None),     # one pixel too wide to stage: gather
    ("f32", 64, 1024, 1, None),     # the widest staged f32 row
    ("u8", 30, 200, 2, None),       # staged rows, upsampled vertically
    ("u8", 60, 179, 1, None),       # last width on the gather path; 180 is the first staged one
    ("u8", 60, 180, 1, None),
]


@pytest.mark.parametrize("dtype,H,W,batch,depth_scale", CASES, ids=[f"{c[0]}-{c[1]}x{c[2]}-b{c[3]}" for c in CASES])
def test_kernel_equals_reference(torch_cuda, engine, dtype, H, W, batch, depth_scale):
    torch = torch_cuda
    raw = _raw(dtype, (batch, H, W), seed=H * 4099 + W)
    want = ingest_reference(raw) if depth_scale is None else ingest_reference(raw, depth_scale)
    dev = torch.from_numpy(raw.view(np.int16) if dtype == "u16" else raw).cuda()
    if dtype == "u16":
        dev = dev.view(torch.uint16)
    _same_bits(_guarded_ingest(torch, engine, dev, batch, depth_scale), want)


def test_f32_half_weights_also_equal_torch(torch_cuda, engine):
    torch = torch_cuda
    raw = _raw("f32", (2, 120, 180), seed=5)
    got = _guarded_ingest(torch, engine, torch.from_numpy(raw).cuda(), 2)
    ref = torch.nn.functional.interpolate(torch.from_numpy(raw)[:, None], size=(60, 90), mode="bilinear",
                                          align_corners=False)[:, 0].numpy()
    _same_bits(got, ref)


def test_int16_is_taken_as_the_same_bits(torch_cuda, engine):
    torch = torch_cuda
    raw = _raw("u16", (2, 240, 320), seed=6)
    got = _guarded_ingest(torch, engine, torch.from_numpy(raw.view(np.int16)).cuda(), 2)      # default scale 1 / 65535
    _same_bits(got, ingest_reference(raw))


def test_cropped_view_is_read_through_its_strides(torch_cuda, engine):
    """460 x 620 view of 480 x 640 frames: row stride 640, frame stride 307200, base offset 10 * 640 + 13 (odd)"""
    torch = torch_cuda
    raw = _raw("u8", (2, 480, 640), seed=7)
    full = torch.from_numpy(raw).cuda()
    view = full[:, 10:470, 13:633]
    assert host.Engine._frame_strides(view) == (640, 480 * 640) and not view.is_contiguous()
    _same_bits(_guarded_ingest(torch, engine, view, 2), ingest_reference(raw[:, 10:470, 13:633]))


@pytest.mark.parametrize("dtype,shape,crop", [("u8", (2, 101, 333), (slice(None), slice(0, 101), slice(1, 332))),
                                              ("u16", (2, 70, 401), (slice(None), slice(3, 70), slice(5, 400))),
                                              ("f32", (2, 63, 203), (slice(None), slice(1, 62), slice(3, 200)))],
                         ids=["u8", "u16", "f32"])
def test_odd_row_strides_change_the_alignment_row_by_row(torch_cuda, engine, dtype, shape, crop):
    """a row stride that is no multiple of 16 bytes: every staged row has another head and tail"""
    torch = torch_cuda
    raw = _raw(dtype, shape, seed=8)
    dev = torch.from_numpy(raw.view(np.int16) if dtype == "u16" else raw).cuda()
    if dtype == "u16":
        dev = dev.view(torch.uint16)
    view = dev[crop]
    assert host.Engine._frame_strides(view) == (shape[2], shape[1] * shape[2])
    _same_bits(_guarded_ingest(torch, engine, view, 2), ingest_reference(raw[crop]))


def test_leading_dimensions_and_forms_that_need_a_copy(torch_cuda, engine):
    torch = torch_cuda
    raw = _raw("u8", (2, 3, 96, 200), seed=9)
    dev = torch.from_numpy(raw).cuda()
    want = ingest_reference(raw)
    assert want.shape == (6, 60, 90)
    _same_bits(_guarded_ingest(torch, engine, dev, 6), want)                                   # (T, B, H, W) collapses
    assert host.Engine._frame_strides(dev[:, 1]) == (200, 3 * 96 * 200)                         # every third frame: one stride
    _same_bits(_guarded_ingest(torch, engine, dev[:, 1], 2), ingest_reference(raw[:, 1]))
    for v, r in ((dev[:, :, :, ::2], raw[:, :, :, ::2]), (dev.transpose(0, 1), raw.transpose(1, 0, 2, 3)),
                 (dev[0, 0].expand(4, 96, 200), np.broadcast_to(raw[0, 0], (4, 96, 200)))):
        assert host.Engine._frame_strides(v) is None                                           # made contiguous first
        _same_bits(_guarded_ingest(torch, engine, v, int(np.prod(r.shape[:-2]))), ingest_reference(np.ascontiguousarray(r)))


def test_more_frames_than_workgroups(torch_cuda, engine):
    """300 frames of 480 x 640: 4500 (frame, row group) items on a grid of 8 workgroups per CU -- every workgroup wraps"""
    torch = torch_cuda
    base = _raw("u8", (4, 480, 640), seed=10)
    idx = (np.arange(300) * 7 + 3) % 4
    dev = torch.from_numpy(base).cuda()[torch.from_numpy(idx).cuda()]
    assert dev.shape == (300, 480, 640) and dev.is_contiguous()
    _same_bits(_guarded_ingest(torch, engine, dev, 300), ingest_reference(base)[idx])


def test_ingest_without_out_allocates_and_returns_n_60_90(torch_cuda, engine):
    torch = torch_cuda
    raw = _raw("u8", (2, 2, 120, 180), seed=11)
    got = engine.ingest(torch.from_numpy(raw).cuda())
    assert tuple(got.shape) == (4, 60, 90) and got.dtype == torch.float32 and got.is_contiguous()
    _same_bits(got.cpu().numpy(), ingest_reference(raw))


def test_forward_of_ingested_frames(torch_cuda, engine, oracle):
    """eng.forward(eng.ingest(raw), desvel) == eng.forward(ingest_reference(raw), desvel) bit for bit, and within the bound
    of tests/test_gpu_parity.py::test_refine_inputs_resize_and_default_quaternion of the oracle on torch's CPU resize
    (tokens 1e-5, velocities 5e-4)"""
    torch = torch_cuda
    rs = np.random.RandomState(21)
    raw = rs.randint(0, 256, size=(2, 120, 180)).astype(np.uint8)
    dv = rs.uniform(2, 8, size=(2, 1)).astype(np.float32)
    ref_frames = ingest_reference(raw)
    v_gpu, (h_gpu, c_gpu), tp = engine.forward(engine.ingest(torch.from_numpy(raw).cuda()), torch.from_numpy(dv).cuda(), taps=True)
    v_ref, (h_ref, c_ref) = engine.forward(torch.from_numpy(ref_frames).cuda(), torch.from_numpy(dv).cuda())
    for a, b in ((v_gpu, v_ref), (h_gpu, h_ref), (c_gpu, c_ref)):
        _same_bits(a.cpu().numpy(), b.cpu().numpy())
    small = torch.nn.functional.interpolate(torch.from_numpy(raw.astype(np.float32) / np.float32(255))[:, None], size=(60, 90),
                                            mode="bilinear", align_corners=False)[:, 0].numpy()
    q = np.zeros((2, 4), np.float32); q[:, 0] = 1
    ov, _, _, otp = oracle.forward(engine.blob, small, dv, q, taps=True)
    np.testing.assert_allclose(tp["tokens"].cpu().numpy(), otp["tokens"], atol=1e-5, rtol=0)
    np.testing.assert_allclose(v_gpu.cpu().numpy(), ov, atol=5e-4, rtol=0)


def test_forward_sequence_of_ingested_frames(torch_cuda, engine, oracle):
    """the same through forward_sequence, T = 2 steps of B = 2 streams"""
    torch = torch_cuda
    rs = np.random.RandomState(22)
    raw = rs.randint(0, 256, size=(2, 2, 120, 180)).astype(np.uint8)
    dv = rs.uniform(2, 8, size=(2, 2)).astype(np.float32)
    ref_frames = ingest_reference(raw).reshape(2, 2, 60, 90)
    got = engine.ingest(torch.from_numpy(raw).cuda()).reshape(2, 2, 60, 90)
    v_gpu, (h_gpu, c_gpu) = engine.forward_sequence(got, torch.from_numpy(dv).cuda())
    v_ref, (h_ref, c_ref) = engine.forward_sequence(torch.from_numpy(ref_frames).cuda(), torch.from_numpy(dv).cuda())
    assert engine.head_status() == 0
    for a, b in ((v_gpu, v_ref), (h_gpu, h_ref), (c_gpu, c_ref)):
        _same_bits(a.cpu().numpy(), b.cpu().numpy())
    small = torch.nn.functional.interpolate(torch.from_numpy(raw.reshape(4, 120, 180).astype(np.float32) / np.float32(255))[:, None],
                                            size=(60, 90), mode="bilinear", align_corners=False)[:, 0].numpy().reshape(2, 2, 60, 90)
    q = np.zeros((2, 4), np.float32); q[:, 0] = 1
    h = c = None
    for t in range(2):
        ov, h, c = oracle.forward(engine.blob, small[t], dv[t].reshape(2, 1), q, h, c)
        np.testing.assert_allclose(v_gpu[t].cpu().numpy(), ov, atol=5e-4, rtol=0)


def test_ingest_refuses_what_it_cannot_run(torch_cuda, engine):
    torch = torch_cuda
    with pytest.raises(host.ITAError):
        engine.ingest(torch.zeros((1, 120, 180), dtype=torch.uint8))                       # a CPU tensor
    if torch.cuda.device_count() > 1:
        with pytest.raises(host.ITAError):
            engine.ingest(torch.zeros((1, 120, 180), dtype=torch.uint8, device="cuda:1"))  # another GPU
    # On a one-GPU box no tensor of another device exists, so the check is reached from the other side: an Engine object
    # that claims the next ordinal.  It is built without __init__ (no context is created on a device that may not exist);
    # ingest compares devices before it uses the handle, and close() / __del__ do nothing with a None handle.
    other = host.Engine.__new__(host.Engine)
    other._h, other.device = None, engine.device + 1
    with pytest.raises(host.ITAError, match="lives on"):
        other.ingest(torch.zeros((1, 120, 180), dtype=torch.uint8, device="cuda:0"))
    for dt in (torch.float16, torch.float64, torch.int32, torch.int8):
        with pytest.raises(host.ITAError):
            engine.ingest(torch.zeros((1, 120, 180), dtype=dt, device="cuda"))
    for shape in ((1, 4097, 8), (1, 8, 4097), (0, 120, 180), (7,)):
        with pytest.raises(host.ITAError):
            engine.ingest(torch.zeros(shape, dtype=torch.uint8, device="cuda"))
    raw = torch.zeros((1, 120, 180), dtype=torch.int16, device="cuda").view(torch.uint16)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(host.ITAError):
            engine.ingest(raw, depth_scale=bad)
    with pytest.raises(host.ITAError):
        engine.ingest(raw, out=torch.empty((2, 60, 90), device="cuda"))                    # out of another shape
