"""The attention-only QAT graph (int8 attention, float32 FFN + residual + LayerNorm2; ITAW0002 blobs) on the MI355X:
ita_ffn_f32 and the fused layer bit-equal to the oracle composition, the whole forward against the composed oracle and
the reference fixtures, the serving forms against the eager forward, and the refusals between the two FFN kinds."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import golden_files
from drone_oa_iree_vit_accelerator_amd import host, params, synth
from gpu_support import cu
from only_attn_common import composed, setup_only_attn as _setup, tensors

pytestmark = pytest.mark.gpu

def _x(B, seed):
    """LayerNorm-like activations (what the FFN sees), with exact zeros and negative values for the ReLU"""
    rs = np.random.RandomState(seed)
    return rs.standard_normal((B, 128, 64)).astype(np.float32)


@pytest.mark.parametrize("L", [1, 2])
def test_ffn_f32_and_layer_bit_equal(oracle, L):
    d, fp, blob = _setup(L)
    t = tensors(d, fp)
    eng = host.Engine(blob, device=0)
    assert [eng.ffn_kind(l) for l in range(L)] == [host.FFN_F32] * L
    for B in (1, 3, 37, 1024):
        x = _x(B, B)
        frames = np.arange(B) if B < 64 else np.random.RandomState(B).choice(B, 24, replace=False)
        for l in range(L):
            y = eng.ffn_f32(cu(x), l).cpu().numpy()
            assert np.array_equal(eng.ffn(cu(x), l).cpu().numpy(), y)
            xs = x[frames]
            hid = np.maximum(oracle.linear_f32(xs, t[f"ffn{l}.w1f"], t[f"ffn{l}.b1f"]), np.float32(0))
            want = oracle.linear_f32(hid, t[f"ffn{l}.w2f"], t[f"ffn{l}.b2f"])
            np.testing.assert_array_equal(y[frames], want, err_msg=f"ffn_f32 B={B} layer {l}")
            # the whole layer: attention + LN1 (int8 blocks) then the float FFN + LN2
            z = eng.encoder_layer(cu(x), l).cpu().numpy()
            x1 = oracle.add_ln(xs, oracle.mha(xs, t, l), t[f"norm1_{l}.w"], t[f"norm1_{l}.b"])
            hid = np.maximum(oracle.linear_f32(x1, t[f"ffn{l}.w1f"], t[f"ffn{l}.b1f"]), np.float32(0))
            want = oracle.add_ln(x1, oracle.linear_f32(hid, t[f"ffn{l}.w2f"], t[f"ffn{l}.b2f"]), t[f"norm2_{l}.w"], t[f"norm2_{l}.b"])
            np.testing.assert_array_equal(z[frames], want, err_msg=f"encoder_layer B={B} layer {l}")
    # in place (y aliases x)
    xx = cu(_x(5, 77))
    want = eng.encoder_layer(xx.clone(), 0)
    host.lib().ita_encoder_layer(eng._h, 0, xx.data_ptr(), xx.data_ptr(), 5, host._stream_ptr(eng.device))
    assert np.array_equal(xx.cpu().numpy(), want.cpu().numpy())
    eng.close()


@pytest.mark.parametrize("L", [1, 2])
@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_forward_against_composed_oracle_and_reference(oracle, L, kind):
    import torch
    d, fp, blob = _setup(L)
    eng = host.Engine(blob, device=0)
    img0 = d["in0.img_u8"] if kind == "u8" else (d["in0.img_u8"].astype(np.float32) / np.float32(255.0))
    img1 = d["in1.img_u8"] if kind == "u8" else (d["in1.img_u8"].astype(np.float32) / np.float32(255.0))
    ov0, oh0, oc0, otp = composed(oracle, d, fp, img0, d["in0.desvel"], d["in0.quat"])
    ov1, oh1, oc1, _ = composed(oracle, d, fp, img1, d["in1.desvel"], d["in1.quat"], oh0, oc0)
    for mode in (0, 1):
        eng.set_tail_mode(mode)
        v0, st, tp = eng.forward(cu(img0), cu(d["in0.desvel"]), cu(d["in0.quat"]), taps=True)
        v1, st1 = eng.forward(cu(img1), cu(d["in1.desvel"]), cu(d["in1.quat"]), st)
        torch.cuda.synchronize()
        for k in ("tokens", "x1", "x2"):
            np.testing.assert_array_equal(tp[k].cpu().numpy(), otp[k], err_msg=f"{k} mode {mode}")
        got = [v0, st[0], st[1], v1, st1[0], st1[1]]
        want = [ov0, oh0, oc0, ov1, oh1, oc1]
        if mode == 0:
            for k in ("feat", "dec"):
                np.testing.assert_array_equal(tp[k].cpu().numpy(), otp[k], err_msg=k)
            for g, w in zip(got, want):
                np.testing.assert_array_equal(g.cpu().numpy(), w)
        else:
            for g, w in zip(got, want):
                assert np.abs(g.cpu().numpy() - w).max() <= 2e-5
        assert np.abs(v0.cpu().numpy() - d["s0.vel"]).max() <= 5e-4
        assert np.abs(v1.cpu().numpy() - d["s1.vel"]).max() <= 5e-4
        assert np.abs(st1[1].cpu().numpy() - d["s1.c"]).max() <= 1e-3
    eng.close()


def test_profiler_stages():
    d, fp, blob = _setup(2)
    eng = host.Engine(blob, device=0)
    fr = synth.frames(3, 8)
    eng.profile_begin(4)
    for _ in range(3):
        eng.forward(cu(fr["img_u8"]), cu(fr["desvel"]), cu(fr["quat"]))
    ms, n = eng.profile_end()
    assert n == 3 and ms["mha"] > 0 and ms["ffn"] > 0
    eng.close()


def test_serving_forms_equal_eager_forward():
    import torch
    _, _, blob = _setup(1)
    eng = host.Engine(blob, device=0)
    # forward_slots with the state updated in place
    B, NS = 5, 16
    fr = synth.frames(21, B)
    img, dv, qt = cu(fr["img_u8"]), cu(fr["desvel"]), cu(fr["quat"])
    rs = np.random.RandomState(0)
    h0 = (0.1 * rs.standard_normal((3, NS, 128))).astype(np.float32)
    c0 = (0.1 * rs.standard_normal((3, NS, 128))).astype(np.float32)
    slots = np.array([7, 0, 15, 3, 9], np.int32)
    sh, sc = cu(h0.copy()), cu(c0.copy())
    vel = eng.forward_slots(img, dv, qt, sh, sc, cu(slots))
    v2, (h2, c2) = eng.forward(img, dv, qt, (cu(h0[:, slots]), cu(c0[:, slots])))
    assert torch.equal(vel, v2)
    assert torch.equal(sh[:, slots.tolist()], h2) and torch.equal(sc[:, slots.tolist()], c2)
    hh, cc = cu(h0[:, slots]), cu(c0[:, slots])
    v3, _ = eng.forward(img, dv, qt, (hh, cc), out=(torch.empty_like(v2), hh, cc))
    assert torch.equal(v3, v2) and torch.equal(hh, h2) and torch.equal(cc, c2)
    # front / back on two streams
    B, T = 37, 3
    frames = [synth.frames(400 + t, B) for t in range(T)]
    ref, hid = [], None
    for t in range(T):
        v, hid = eng.forward(cu(frames[t]["img_u8"]), cu(frames[t]["desvel"]), cu(frames[t]["quat"]), hid)
        ref.append((v.clone(), hid[0].clone(), hid[1].clone()))
    sf, sb = torch.cuda.Stream(), torch.cuda.Stream()
    state = [(torch.zeros((3, B, 128), device="cuda"), torch.zeros((3, B, 128), device="cuda")) for _ in range(2)]
    torch.cuda.synchronize()
    for t in range(T):
        ev = torch.cuda.Event()
        eng.front(cu(frames[t]["img_u8"]), 0, stream=sf)
        ev.record(sf)
        sb.wait_event(ev)
        out = torch.empty((B, 3), device="cuda")
        dst = state[(t + 1) & 1]
        eng.back(cu(frames[t]["desvel"]).reshape(B), cu(frames[t]["quat"]), state[t & 1], (out, dst[0], dst[1]), 0, stream=sb)
        sb.synchronize()
        assert torch.equal(out, ref[t][0]) and torch.equal(dst[0], ref[t][1]) and torch.equal(dst[1], ref[t][2]), t
    del out, dst
    # graphed step
    g = eng.graphed_step(B)
    st = (torch.zeros((3, B, 128), device="cuda"), torch.zeros((3, B, 128), device="cuda"))
    for t in range(T):
        g.img.copy_(cu(frames[t]["img_u8"])); g.desvel.copy_(cu(frames[t]["desvel"]).reshape(B)); g.quat.copy_(cu(frames[t]["quat"]))
        vg = g().clone()
        ve, st = eng.forward(cu(frames[t]["img_u8"]), cu(frames[t]["desvel"]), cu(frames[t]["quat"]), st)
        assert torch.equal(vg, ve) and torch.equal(g.h, st[0]) and torch.equal(g.c, st[1]), t
    del g
    eng.close()


@pytest.mark.parametrize("stages", [2, 3])
def test_pipelined_steps_equal_sequential_forward(stages):
    import torch
    _, _, blob = _setup(2)
    eng = host.Engine(blob, device=0)
    B, n = 3, 8
    frs = [synth.frames(500 + t, B) for t in range(n)]
    ps = eng.pipelined_steps(B, n, stages)
    for t in range(n):
        ps.img[t].copy_(torch.from_numpy(frs[t]["img_u8"]))
        ps.desvel[t].copy_(torch.from_numpy(frs[t]["desvel"]).reshape(B))
        ps.quat[t].copy_(torch.from_numpy(frs[t]["quat"]))
    got = ps().clone()
    torch.cuda.synchronize()
    eng2 = host.Engine(blob, device=0)
    st = None
    for t in range(n):
        v, st = eng2.forward(cu(frs[t]["img_u8"]), cu(frs[t]["desvel"]), cu(frs[t]["quat"]), st)
        assert torch.equal(got[t], v), t
    assert torch.equal(ps.h, st[0]) and torch.equal(ps.c, st[1])
    del ps
    eng.close(); eng2.close()


def test_udp_server_end_to_end(oracle):
    """the sample server on an ITAW0002 blob: replies equal the composed oracle's pipeline"""
    import socket, struct, subprocess, tempfile
    d, fp, blob = _setup(1)
    exe = host.build_samples()
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    nclients, steps = 2, 2
    with tempfile.NamedTemporaryFile(suffix=".itaw") as f:
        f.write(blob); f.flush()
        srv = subprocess.Popen([exe, "--blob", f.name, "--port", str(port), "--max-packets", str(nclients * steps),
                                "--max-streams", "8", "--max-batch", "8"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                               text=True)
        try:
            assert "listening" in srv.stdout.readline()
            socks = [socket.socket(socket.AF_INET, socket.SOCK_DGRAM) for _ in range(nclients)]
            for sk in socks:
                sk.settimeout(30)
            h = [None] * nclients
            c = [None] * nclients
            for t in range(steps):
                fr = synth.frames(300 + t, nclients)
                posx = [0.5, 30.0]
                for i, sk in enumerate(socks):
                    pk = fr["img_u8"][i].tobytes() + struct.pack(">ff", float(fr["desvel"][i, 0]), posx[i]) + \
                        struct.pack(">4f", *[float(q) for q in fr["quat"][i]])
                    sk.sendto(pk, ("127.0.0.1", port))
                for i, sk in enumerate(socks):
                    got = np.frombuffer(sk.recvfrom(64)[0], "<f4")
                    dv = np.float32(fr["desvel"][i, 0])
                    vel, h[i], c[i], _ = composed(oracle, d, fp, fr["img_u8"][i:i + 1], np.array([[dv / np.float32(10.0)]], np.float32),
                                                  fr["quat"][i:i + 1], h[i], c[i])
                    np.testing.assert_allclose(got, oracle.final_velocity(vel[0], float(dv), posx[i]), atol=3e-4, rtol=0)
            out, _ = srv.communicate(timeout=60)
            assert srv.returncode == 0, out
        finally:
            if srv.poll() is None:
                srv.kill()


def test_refusals_between_ffn_kinds():
    import torch
    _, _, blob = _setup(1)
    fx = params.load_fixture(golden_files("vitlstm_E64_seed0_B2.npz")[0])
    b8 = params.blob_from_record(fx, synth.float_params(0, E=64), E=64)
    L = host.lib()
    e32, e8 = host.Engine(blob, device=0), host.Engine(b8, device=0)
    assert e32.ffn_kind(0) == host.FFN_F32 and e8.ffn_kind(0) == host.FFN_INT8
    x = cu(_x(2, 1))
    y = torch.empty_like(x)
    s = host._stream_ptr(0)
    assert L.ita_ffn_int8(e32._h, 0, x.data_ptr(), y.data_ptr(), 2, s) == -4
    assert L.ita_ffn_int8_taps(e32._h, 0, x.data_ptr(), y.data_ptr(), 2, None, s) == -4
    assert L.ita_ffn_f32(e8._h, 0, x.data_ptr(), y.data_ptr(), 2, s) == -4
    with pytest.raises(host.ITAError):
        e32.ffn(x, 0, taps=True)
    # the drop-in symbol bound to a float layer reports through ita_last_error
    e32.bind_dispatch(0, host.DISPATCH_F32)
    buf = np.zeros(128 * 64, np.float32)
    out = np.zeros_like(buf)
    L.ITAFeedForward_workgroup(buf.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    assert L.ita_last_error() == -4
    e8.bind_dispatch(0, host.DISPATCH_F32)
    L.ITAFeedForward_workgroup(buf.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    assert L.ita_last_error() == 0
    e32.close(); e8.close()
