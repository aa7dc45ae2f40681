"""The wire ingest kernel (ita_ingest_wire / Engine.ingest_wire) against its definition,
ingest_wire_ref.ingest_wire_reference: bit for bit, on every size of the stb fixtures and on every stride form and table
class the entry accepts, with a 90-byte guard of a sentinel code in front of and behind the (N,60,90) output.  Then the
entry's refusals, and end to end: ingested frames through forward / forward_sequence on the u8 wire path."""
import numpy as np
import pytest

from conftest import golden_files
from drone_oa_iree_vit_accelerator_amd import host, params, synth
from drone_oa_iree_vit_accelerator_amd.ingest_wire_ref import ingest_wire_reference

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
SIZES = ["96x128", "480x640", "720x1280", "61x93", "30x45", "100x64", "1x200", "200x1", "1x1", "8x4096", "4096x8"]
ORACLE_TOL = 2e-5     # tests/test_gpu_parity.py, u8 frames, tail mode 1: velocities and state against the oracle


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def engine(torch_cuda):
    fx = params.load_fixture(golden_files("vitlstm_E64_seed0_B2.npz")[0])
    blob = params.blob_from_record(fx, synth.float_params(0, E=64), E=64)
    eng = host.Engine(blob, device=0, reserve=8)
    eng.blob = blob
    yield eng
    eng.close()


def _raw(shape, seed):
    return np.random.RandomState(seed).randint(0, 256, size=shape).astype(np.uint8)


def _guarded(torch, eng, frames, n):
    """Engine.ingest_wire into the middle of a sentinel-filled buffer with a 90-byte guard on each side -> numpy"""
    buf = torch.full((n * 60 + 2, 90), SENTINEL, dtype=torch.uint8, device="cuda")
    out = buf[1:-1].view(n, 60, 90)
    got = eng.ingest_wire(frames, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    host_buf = buf.cpu().numpy()
    assert (host_buf[0] == SENTINEL).all() and (host_buf[-1] == SENTINEL).all(), "a guard was written"
    return host_buf[1:-1].reshape(n, 60, 90)


def _same(got, want):
    assert got.dtype == np.uint8 and want.dtype == np.uint8 and got.shape == want.shape
    diff = got != want
    assert not diff.any(), f"{int(diff.sum())} of {diff.size} codes differ, first at {tuple(np.argwhere(diff)[0])}"


@pytest.mark.parametrize("size", SIZES)
def test_kernel_equals_definition_on_the_fixture_frames(torch_cuda, engine, size):
    """the five frames of each stb fixture (noise, field, flat blocks, all-255, 0/255 noise)"""
    src = np.load(golden_files(f"resize_stb_{size}.npz")[0])["src"]
    _same(_guarded(torch_cuda, engine, torch_cuda.from_numpy(src).cuda(), len(src)), ingest_wire_reference(src))


def test_frame_stride_larger_than_the_frame(torch_cuda, engine):
    """a batch of 3 whose frames lie 1000 bytes further apart than they are long (row stride 128: aligned dwords)"""
    torch = torch_cuda
    raw = _raw((3, 96 * 128 + 1000), 1)
    view = torch.from_numpy(raw).cuda()[:, :96 * 128].view(3, 96, 128)
    assert host.Engine._frame_strides(view) == (128, 96 * 128 + 1000) and not view.is_contiguous()
    _same(_guarded(torch, engine, view, 3), ingest_wire_reference(raw[:, :96 * 128].reshape(3, 96, 128)))


def test_cropped_view_at_an_odd_offset_with_an_odd_row_stride(torch_cuda, engine):
    """99 x 321 view of 101 x 333 frames at byte offset 333 + 6 = 339: the alignment changes row by row (pixel-by-pixel
    path)"""
    torch = torch_cuda
    raw = _raw((2, 101, 333), 2)
    full = torch.from_numpy(raw).cuda()
    view = full[:, 1:100, 6:327]
    assert host.Engine._frame_strides(view) == (333, 101 * 333) and view.data_ptr() - full.data_ptr() == 339
    _same(_guarded(torch, engine, view, 2), ingest_wire_reference(raw[:, 1:100, 6:327]))


@pytest.mark.parametrize("off", [1, 2, 3])
def test_cropped_view_with_an_aligned_row_stride(torch_cuda, engine, off):
    """460 x 615 view of 480 x 640 frames starting `off` bytes into a row: aligned dwords with single pixels in front of
    the first and behind the last one"""
    torch = torch_cuda
    raw = _raw((2, 480, 640), 3)
    view = torch.from_numpy(raw).cuda()[:, 10:470, off:off + 615]
    assert host.Engine._frame_strides(view) == (640, 480 * 640)
    _same(_guarded(torch, engine, view, 2), ingest_wire_reference(raw[:, 10:470, off:off + 615]))


@pytest.mark.parametrize("H,W,batch", [(480, 640, 2), (8, 4096, 1), (4096, 8, 1), (2, 3, 2), (60, 90, 2), (64, 7, 1)],
                         ids=lambda v: str(v))
def test_random_frames(torch_cuda, engine, H, W, batch):
    """the real shape, the widest row and the tallest column (274 vertical taps), rows shorter than a dword, the identity"""
    raw = _raw((batch, H, W), H * 4099 + W)
    got = _guarded(torch_cuda, engine, torch_cuda.from_numpy(raw).cuda(), batch)
    _same(got, ingest_wire_reference(raw))
    if (H, W) == (60, 90):
        _same(got, raw)


def test_more_items_than_workgroups(torch_cuda, engine):
    """600 frames of 96 x 128: 9000 (frame, four rows) items on a grid of 8 workgroups per CU -- every workgroup wraps"""
    torch = torch_cuda
    base = _raw((4, 96, 128), 5)
    idx = (np.arange(600) * 7 + 3) % 4
    dev = torch.from_numpy(base).cuda()[torch.from_numpy(idx).cuda()]
    _same(_guarded(torch, engine, dev, 600), ingest_wire_reference(base)[idx])


def test_unprepared_then_prepared_and_more_sizes_than_the_cache_holds(torch_cuda, engine):
    torch = torch_cuda
    raw = _raw((1, 75, 100), 6)
    dev, want = torch.from_numpy(raw).cuda(), ingest_wire_reference(raw)
    _same(_guarded(torch, engine, dev, 1), want)              # prepares on first use
    engine.prepare_ingest_wire(75, 100)                        # already there: nothing happens
    _same(_guarded(torch, engine, dev, 1), want)
    for k in range(10):                                        # ten further sizes push 75 x 100 out of the eight slots
        engine.prepare_ingest_wire(40 + k, 50 + k)
    _same(_guarded(torch, engine, dev, 1), want)               # and it is built again
    small = _raw((1, 45, 55), 7)
    _same(_guarded(torch, engine, torch.from_numpy(small).cuda(), 1), ingest_wire_reference(small))


def test_leading_dimensions_allocation_and_forms_that_need_a_copy(torch_cuda, engine):
    torch = torch_cuda
    raw = _raw((2, 3, 96, 200), 8)
    dev = torch.from_numpy(raw).cuda()
    got = engine.ingest_wire(dev)
    assert tuple(got.shape) == (6, 60, 90) and got.dtype == torch.uint8 and got.is_contiguous()
    _same(got.cpu().numpy(), ingest_wire_reference(raw))
    for v, r in ((dev[:, :, :, ::2], raw[:, :, :, ::2]), (dev.transpose(0, 1), raw.transpose(1, 0, 2, 3))):
        assert host.Engine._frame_strides(v) is None
        _same(_guarded(torch, engine, v, 6), ingest_wire_reference(np.ascontiguousarray(r)))


def test_argument_errors(torch_cuda, engine):
    """every rule of the header returns ITA_ERR_INVALID_ARG; the output keeps its sentinel"""
    torch = torch_cuda
    L = host.lib()
    src = torch.zeros((2, 480, 640), dtype=torch.uint8, device="cuda")
    dst = torch.full((2, 60, 90), SENTINEL, dtype=torch.uint8, device="cuda")
    good = dict(h=engine._h, src=src.data_ptr(), H=480, W=640, rs=640, fs=480 * 640, dst=dst.data_ptr(), batch=2)

    def call(**kw):
        a = dict(good, **kw)
        return L.ita_ingest_wire(a["h"], a["src"], a["H"], a["W"], a["rs"], a["fs"], a["dst"], a["batch"], None)

    for kw in (dict(h=None), dict(src=None), dict(dst=None), dict(H=0), dict(H=4097), dict(W=0), dict(W=4097), dict(rs=639),
               dict(fs=479 * 640 + 639), dict(rs=(1 << 40) + 4, fs=1 << 62), dict(fs=(1 << 40) + 1), dict(batch=0),
               dict(batch=-1)):
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert (dst == SENTINEL).all()
    with pytest.raises(host.ITAError):
        engine.ingest_wire(torch.zeros((1, 96, 128), dtype=torch.uint8))                     # a CPU tensor
    for dt in (torch.float32, torch.int16, torch.int8):
        with pytest.raises(host.ITAError):
            engine.ingest_wire(torch.zeros((1, 96, 128), dtype=dt, device="cuda"))
    for shape in ((1, 4097, 8), (1, 8, 4097), (0, 96, 128), (7,)):
        with pytest.raises(host.ITAError):
            engine.ingest_wire(torch.zeros(shape, dtype=torch.uint8, device="cuda"))
    with pytest.raises(host.ITAError):
        engine.ingest_wire(src, out=torch.empty((3, 60, 90), dtype=torch.uint8, device="cuda"))
    with pytest.raises(host.ITAError):
        engine.prepare_ingest_wire(0, 640)


def test_capture_takes_a_prepared_size_and_refuses_an_unprepared_one(torch_cuda, engine):
    """inside torch.cuda.graph: a prepared size is captured and replays; a size without tables is refused before any
    launch (its tables would have to be allocated), and its output keeps the sentinel"""
    torch = torch_cuda
    raw = _raw((2, 96, 128), 9)
    dev = torch.from_numpy(raw).cuda()
    out1 = torch.full((2, 60, 90), SENTINEL, dtype=torch.uint8, device="cuda")
    out2 = torch.full((1, 60, 90), SENTINEL, dtype=torch.uint8, device="cuda")
    other = torch.zeros((1, 77, 131), dtype=torch.uint8, device="cuda")
    engine.prepare_ingest_wire(96, 128)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        engine.ingest_wire(dev, out=out1)                      # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    out1.fill_(SENTINEL)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    refused = None
    with torch.cuda.graph(g):
        engine.ingest_wire(dev, out=out1)
        try:
            engine.ingest_wire(other, out=out2)
        except host.ITAError as e:
            refused = e
    assert refused is not None and "capture" in str(refused)
    g.replay()
    torch.cuda.synchronize()
    _same(out1.cpu().numpy(), ingest_wire_reference(raw))
    assert (out2 == SENTINEL).all()
    del g


def test_forward_of_ingested_frames(torch_cuda, engine, oracle):
    """eng.forward(eng.ingest_wire(raw), desvel) at 96 x 128, B = 2: equal to eng.forward on the definition's codes bit for
    bit, and to oracle.forward on those codes within the bound of tests/test_gpu_parity.py for u8 frames"""
    torch = torch_cuda
    rs = np.random.RandomState(21)
    raw = rs.randint(0, 256, size=(2, 96, 128)).astype(np.uint8)
    dv = rs.uniform(2, 8, size=(2, 1)).astype(np.float32)
    codes = ingest_wire_reference(raw)
    wire = engine.ingest_wire(torch.from_numpy(raw).cuda())
    assert wire.dtype == torch.uint8
    v_gpu, (h_gpu, c_gpu) = engine.forward(wire, torch.from_numpy(dv).cuda())
    v_ref, (h_ref, c_ref) = engine.forward(torch.from_numpy(codes).cuda(), torch.from_numpy(dv).cuda())
    for a, b in ((v_gpu, v_ref), (h_gpu, h_ref), (c_gpu, c_ref)):
        np.testing.assert_array_equal(a.cpu().numpy(), b.cpu().numpy())
    q = np.zeros((2, 4), np.float32); q[:, 0] = 1
    ov, oh, oc = oracle.forward(engine.blob, codes, dv, q)
    for name, got, want in (("vel", v_gpu, ov), ("h", h_gpu, oh), ("c", c_gpu, oc)):
        err = float(np.abs(got.cpu().numpy() - want).max())
        print(f"max |{name} - oracle| = {err:.3e}")
        assert err <= ORACLE_TOL, name


def test_forward_sequence_of_ingested_frames(torch_cuda, engine, oracle):
    """the same through forward_sequence, T = 3 steps of B = 2 streams"""
    torch = torch_cuda
    rs = np.random.RandomState(22)
    raw = rs.randint(0, 256, size=(3, 2, 96, 128)).astype(np.uint8)
    dv = rs.uniform(2, 8, size=(3, 2)).astype(np.float32)
    codes = ingest_wire_reference(raw).reshape(3, 2, 60, 90)
    wire = engine.ingest_wire(torch.from_numpy(raw).cuda()).reshape(3, 2, 60, 90)
    v_gpu, (h_gpu, c_gpu) = engine.forward_sequence(wire, torch.from_numpy(dv).cuda())
    v_ref, (h_ref, c_ref) = engine.forward_sequence(torch.from_numpy(codes).cuda(), torch.from_numpy(dv).cuda())
    assert engine.head_status() == 0
    for a, b in ((v_gpu, v_ref), (h_gpu, h_ref), (c_gpu, c_ref)):
        np.testing.assert_array_equal(a.cpu().numpy(), b.cpu().numpy())
    q = np.zeros((2, 4), np.float32); q[:, 0] = 1
    h = c = None
    for t in range(3):
        ov, h, c = oracle.forward(engine.blob, codes[t], dv[t].reshape(2, 1), q, h, c)
        err = float(np.abs(v_gpu[t].cpu().numpy() - ov).max())
        print(f"step {t}: max |vel - oracle| = {err:.3e}")
        assert err <= ORACLE_TOL, t
    assert float(np.abs(h_gpu.cpu().numpy() - h).max()) <= ORACLE_TOL and float(np.abs(c_gpu.cpu().numpy() - c).max()) <= ORACLE_TOL
