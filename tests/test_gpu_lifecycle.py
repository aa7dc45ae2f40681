"""Handle lifecycle through the raw C ABI (run with -m gpu on the MI355X box): reloading weights across graph families
on one handle, a failed load, and create / load / run / destroy cycles.  Everything here is host-side bookkeeping of the
plugin -- which device buffers a handle owns and when they are rebuilt or released -- so the bars are equality of the
forward's outputs across reloads, the ABI's status codes, and the device's free memory."""
import ctypes

import numpy as np
import pytest

from conftest import golden_files
from drone_oa_iree_vit_accelerator_amd import host, params, synth

pytestmark = pytest.mark.gpu

B = 2
NO_WEIGHTS, BAD_BLOB = -3, -2


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _create():
    h = ctypes.c_void_p()
    assert host.lib().ita_create(ctypes.byref(h), 0) == 0
    return h


def _load(h, blob, nbytes=None):
    buf = ctypes.create_string_buffer(blob, len(blob))
    return host.lib().ita_load_weights(h, buf, len(blob) if nbytes is None else nbytes)


def _forward(torch, h, d):
    """ita_vitlstm_forward on the fixture's first step, zero state; returns (vel, h, c) as numpy"""
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    img, dv, qt = cu(d["in0.img_u8"][:B]), cu(d["in0.desvel"][:B]), cu(d["in0.quat"][:B])
    h_in, c_in = torch.zeros((3, B, 128), device="cuda"), torch.zeros((3, B, 128), device="cuda")
    vel, h_out, c_out = torch.empty((B, 3), device="cuda"), torch.empty_like(h_in), torch.empty_like(c_in)
    torch.cuda.synchronize()
    rc = host.lib().ita_vitlstm_forward(h, img.data_ptr(), host.IMAGE_U8, dv.data_ptr(), qt.data_ptr(), h_in.data_ptr(),
                                        c_in.data_ptr(), vel.data_ptr(), h_out.data_ptr(), c_out.data_ptr(), B, None, None)
    assert rc == 0, host.lib().ita_error_string()
    torch.cuda.synchronize()
    return vel.cpu().numpy(), h_out.cpu().numpy(), c_out.cpu().numpy()


@pytest.fixture(scope="module")
def first_runs(torch_cuda):
    """One handle; the E = 64 ViT+LSTM blob and the two-layer E = 128 blob each loaded and run once on it.  The outputs
    are the reference of every test below and are not modified."""
    d64 = params.load_fixture(golden_files("vitlstm_E64_seed0_B2.npz")[0])
    blob64 = params.blob_from_record(d64, synth.float_params(0, E=64), E=64)
    d128 = params.load_fixture(golden_files("vit2l_E128_s0_B2.npz")[0])      # as test_two_layer_e128_no_tail_graph builds it
    nl = int(d128["meta.num_layers"])
    blob128 = params.blob_from_record(d128, synth.float_params(int(d128["meta.seed"]), E=128, num_layers=nl, tail=False),
                                      E=128, num_layers=nl)
    h = _create()
    assert _load(h, blob64) == 0
    out64 = _forward(torch_cuda, h, d64)
    assert _load(h, blob128) == 0
    out128 = _forward(torch_cuda, h, d128)
    yield {"h": h, "d64": d64, "blob64": blob64, "out64": out64, "d128": d128, "blob128": blob128, "out128": out128}
    assert host.lib().ita_destroy(h) == 0


def _assert_same(got, want, what):
    for g, w, name in zip(got, want, ("vel", "h", "c")):
        np.testing.assert_array_equal(g, w, err_msg=f"{what}: {name}")


def test_reload_across_graph_families(torch_cuda, first_runs):
    """E = 64 with a fusion tail (K = 8192 folded GEMM) and E = 128 without one (K = 16384), alternately on one handle:
    weights, workspace and fold are rebuilt with a changed E, kfold and ldfold, and every forward equals its first run."""
    r = first_runs
    for n in (1, 2):
        assert _load(r["h"], r["blob64"]) == 0
        _assert_same(_forward(torch_cuda, r["h"], r["d64"]), r["out64"], f"E = 64, reload {n}")
        assert _load(r["h"], r["blob128"]) == 0
        _assert_same(_forward(torch_cuda, r["h"], r["d128"]), r["out128"], f"E = 128, reload {n}")


def test_failed_load_unloads_the_handle(torch_cuda, first_runs):
    """Both failures are host-side validation: the header check, and the tensor table check on a blob cut in half."""
    r, lib = first_runs, host.lib()
    blob = r["blob64"]
    garbage = b"NOTABLOB" + b"\0" * 128
    x = torch_cuda.zeros((B, 128, 64), device="cuda")
    h = _create()
    for what, bad, nbytes in (("garbage header", garbage, 136), ("truncated blob", blob, len(blob) // 2)):
        assert _load(h, blob) == 0
        assert _load(h, bad, nbytes) == BAD_BLOB, what
        assert lib.ita_mha_int8(h, 0, x.data_ptr(), x.data_ptr(), B, None) == NO_WEIGHTS, what
        assert _load(h, blob) == 0, what
        _assert_same(_forward(torch_cuda, h, r["d64"]), r["out64"], f"after the {what}")
    assert lib.ita_destroy(h) == 0


def test_cycles_do_not_leak_a_plane(torch_cuda, first_runs):
    """Four create / load / reserve / forward / ita_fusion_tail_load / destroy cycles lower the device's free memory by
    less than one folded-weight plane, 512 x (8192 + 64) f16.  One load allocates more than four such planes (two fold
    planes, their two fragment copies, the blob, the workspace), so a leak of that order shows many times over.  A leak
    much smaller than a plane -- a bias vector, a stream image -- is below what the allocator's accounting can show
    and out of this test's reach."""
    r, lib = first_runs, host.lib()
    E, CO = 128, 48
    rs = np.random.RandomState(7)
    conv_w = (rs.standard_normal((CO, E // 4 + E, 3, 3)) * 0.05).astype(np.float32)
    conv_b = rs.standard_normal(CO).astype(np.float32)

    def cycle():
        h = _create()
        assert _load(h, r["blob64"]) == 0
        assert lib.ita_reserve(h, B) == 0
        _forward(torch_cuda, h, r["d64"])
        assert lib.ita_fusion_tail_load(h, conv_w.ctypes.data_as(ctypes.c_void_p), conv_b.ctypes.data_as(ctypes.c_void_p),
                                        E, CO) == 0
        assert lib.ita_destroy(h) == 0

    cycle()
    torch_cuda.cuda.synchronize()
    free0 = torch_cuda.cuda.mem_get_info()[0]
    for _ in range(4):
        cycle()
    torch_cuda.cuda.synchronize()
    free1 = torch_cuda.cuda.mem_get_info()[0]
    plane = 512 * (8192 + 64) * 2
    print(f"free memory before / after four cycles: {free0} / {free1} bytes, drop {free0 - free1}, bound {plane}")
    assert free0 - free1 < plane
