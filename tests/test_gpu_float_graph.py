"""The float ViT+LSTM graph (ITAW0003 blobs: float32 attention with a true softmax, float32 FFN) on the MI355X:
ita_mha_f32 against a float64 restatement of models/ITA/layers.py:67-88, whole layers and forwards against the
reference's float module (tests/golden/floattwin*) and FloatTwin, the serving forms against the eager forward, the
float-checkpoint path, and the refusals between the attention kinds."""
import ctypes as C

import numpy as np
import pytest

from conftest import golden_files
from drone_oa_iree_vit_accelerator_amd import float_twin, host, params, synth
from gpu_support import cu
from float_graph_common import attn64, float_state_dict, ln_like, setup_float as _setup

pytestmark = pytest.mark.gpu

def test_mha_f32_against_float64():
    """On the reference's tokens (|logit| <= 109) within 1e-5 of float64.  The random activations reach |logit| ~ 230,
    where torch's own f32 attention is 1.3e-5 .. 3.1e-5 off float64: there the bound is three times torch's f32 error
    on the same frames (and never below 1e-5)."""
    import torch
    worst = {}
    for L in (1, 2):
        d, fp, blob = _setup(L)
        eng = host.Engine(blob, device=0)
        twin = float_twin.FloatTwin(fp, num_layers=L)
        assert [eng.attn_kind(l) for l in range(L)] == [host.ATTN_F32] * L
        assert [eng.ffn_kind(l) for l in range(L)] == [host.FFN_F32] * L
        cases = [("tokens", d["s0.tok.out"])] + [(f"ln B={B}", ln_like(B, B, 64)) for B in (1, 3, 37, 1024)]
        for name, x in cases:
            B = x.shape[0]
            frames = np.arange(B) if B < 64 else np.random.RandomState(B).choice(B, 24, replace=False)
            for l in range(L):
                y = eng.mha_f32(cu(x), l).cpu().numpy()
                assert np.array_equal(eng.mha(cu(x), l).cpu().numpy(), y)
                want = attn64(x[frames], fp, l)
                err = np.abs(y[frames] - want).max()
                terr = np.abs(twin._attention(torch.from_numpy(x[frames]), l).numpy() - want).max()
                worst[(name, L, l)] = (float(err), float(terr))
                bound = 1e-5 if name == "tokens" else max(1e-5, 3 * terr)
                assert err <= bound, (name, L, l, err, terr)
        eng.close()
    for k, (e, t) in worst.items():
        print(f"mha_f32 {k}: |gpu - float64| = {e:.3e}, |torch f32 - float64| = {t:.3e}")


def test_frames_independent_and_runs_repeatable():
    _, _, blob = _setup(1)
    eng = host.Engine(blob, device=0)
    x = ln_like(37, 5, 64)
    y = eng.mha_f32(cu(x), 0).cpu().numpy()
    assert np.array_equal(eng.mha_f32(cu(x), 0).cpu().numpy(), y)
    z = eng.encoder_layer(cu(x), 0).cpu().numpy()
    assert np.array_equal(eng.encoder_layer(cu(x), 0).cpu().numpy(), z)
    for b in (0, 17, 36):
        assert np.array_equal(eng.mha_f32(cu(x[b:b + 1]), 0).cpu().numpy()[0], y[b]), b
        assert np.array_equal(eng.encoder_layer(cu(x[b:b + 1]), 0).cpu().numpy()[0], z[b]), b
    # in place (y aliases x)
    xx = cu(x)
    host.lib().ita_encoder_layer(eng._h, 0, xx.data_ptr(), xx.data_ptr(), 37, host._stream_ptr(eng.device))
    assert np.array_equal(xx.cpu().numpy(), z)
    eng.close()


@pytest.mark.parametrize("L", [1, 2])
def test_layers_from_reference_tokens(L):
    d, fp, blob = _setup(L)
    eng = host.Engine(blob, device=0)
    x = cu(d["s0.tok.out"])
    for l in range(L):
        x = eng.encoder_layer(x, l)
        want = d[f"s0.x2_{l}"] if L > 1 else d["s0.x2"]
        err = np.abs(x.cpu().numpy() - want).max()
        assert err <= 2e-5, (l, err)
    # the forward's x1 tap (LayerNorm1 output of the last layer) from the u8 frames
    _, _, tp = eng.forward(cu(d["in0.img_u8"]), cu(d["in0.desvel"]), cu(d["in0.quat"]), taps=True)
    assert np.abs(tp["x1"].cpu().numpy() - d["s0.x1"]).max() <= 2e-5
    eng.close()


@pytest.mark.parametrize("L", [1, 2])
def test_forward_against_reference_and_float_twin(L):
    import torch
    d, fp, blob = _setup(L)
    eng = host.Engine(blob, device=0)
    twin = float_twin.FloatTwin(fp, num_layers=L)
    fr = synth.frames(60 + L, 64)
    tv0, tst0, ttp = twin.forward(fr["img_u8"], fr["desvel"], fr["quat"], taps=True)
    rs = np.random.RandomState(L)
    hid = tuple((0.1 * rs.standard_normal((3, 64, 128))).astype(np.float32) for _ in range(2))
    tv1, tst1 = twin.forward(fr["img_u8"], fr["desvel"], fr["quat"], hidden=hid)
    for mode in (0, 1):
        eng.set_tail_mode(mode)
        v0, st, tp = eng.forward(cu(d["in0.img_u8"]), cu(d["in0.desvel"]), cu(d["in0.quat"]), taps=True)
        v1, st1 = eng.forward(cu(d["in1.img_u8"]), cu(d["in1.desvel"]), cu(d["in1.quat"]), st)
        torch.cuda.synchronize()
        assert np.abs(tp["tokens"].cpu().numpy() - d["s0.tok.out"]).max() <= 2e-5
        for k in ("x1", "x2") + (("dec",) if mode == 0 else ()):
            err = np.abs(tp[k].cpu().numpy() - d["s0." + k]).max()
            assert err <= 1e-4, (mode, k, err)
        for g, k in ((v0, "s0.vel"), (st[0], "s0.h"), (st[1], "s0.c"), (v1, "s1.vel"), (st1[0], "s1.h"), (st1[1], "s1.c")):
            err = np.abs(g.cpu().numpy() - d[k]).max()
            assert err <= 5e-4, (mode, k, err)
        # FloatTwin on the CPU, 64 frames, zero and given state
        g0, gst, gtp = eng.forward(cu(fr["img_u8"]), cu(fr["desvel"]), cu(fr["quat"]), taps=True)
        g1, gst1 = eng.forward(cu(fr["img_u8"]), cu(fr["desvel"]), cu(fr["quat"]), (cu(hid[0]), cu(hid[1])))
        assert np.abs(gtp["tokens"].cpu().numpy() - ttp["tokens"].numpy()).max() <= 2e-5
        for k in ("x1", "x2") + (("dec",) if mode == 0 else ()):
            err = np.abs(gtp[k].cpu().numpy() - ttp[k].numpy()).max()
            assert err <= 1e-4, (mode, k, err)
        for g, w in ((g0, tv0), (gst[0], tst0[0]), (gst[1], tst0[1]), (g1, tv1), (gst1[0], tst1[0]), (gst1[1], tst1[1])):
            assert np.abs(g.cpu().numpy() - w.numpy()).max() <= 5e-4
    eng.close()


def test_profiler_stages():
    _, _, blob = _setup(2)
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


def test_float_checkpoint_runs():
    sd = float_state_dict(1, 3)
    blob = params.blob_from_state_dict(sd, 1)
    fp = synth.float_params(3, E=64)
    fp["decoder.weight"] = params.fold_spectral_norm(sd, "decoder")
    fp["nn_fc2.weight"] = params.fold_spectral_norm(sd, "nn_fc2")
    fr = synth.frames(9, 16)
    eng, eng2 = host.Engine(blob, device=0), host.Engine(params.blob_from_float_params(fp), device=0)
    v, _ = eng.forward(cu(fr["img_u8"]), cu(fr["desvel"]), cu(fr["quat"]))
    v2, _ = eng2.forward(cu(fr["img_u8"]), cu(fr["desvel"]), cu(fr["quat"]))
    assert np.abs(v.cpu().numpy() - v2.cpu().numpy()).max() <= 1e-5
    tv, _ = float_twin.FloatTwin(fp).forward(fr["img_u8"], fr["desvel"], fr["quat"])
    assert np.abs(v.cpu().numpy() - tv.numpy()).max() <= 5e-4
    eng.close(); eng2.close()


def test_refusals_between_attention_kinds():
    import torch
    _, _, blob = _setup(1)
    fx = params.load_fixture(golden_files("vitlstm_E64_seed0_B2.npz")[0])
    b8 = params.blob_from_record(fx, synth.float_params(0, E=64), E=64)
    L = host.lib()
    ef, e8 = host.Engine(blob, device=0), host.Engine(b8, device=0)
    assert ef.attn_kind(0) == host.ATTN_F32 and e8.attn_kind(0) == host.ATTN_INT8
    x = cu(ln_like(2, 1, 64))
    y = torch.empty_like(x)
    xq = torch.zeros((2, 128, 64), dtype=torch.int8, device="cuda")
    yq = torch.empty_like(xq)
    img = cu(fx["in0.img_u8"])
    stamps = torch.zeros(4096, dtype=torch.int64, device="cuda")
    s = host._stream_ptr(0)
    assert L.ita_mha_int8(ef._h, 0, x.data_ptr(), y.data_ptr(), 2, s) == -4
    assert L.ita_mha_int8_taps(ef._h, 0, x.data_ptr(), y.data_ptr(), 2, None, s) == -4
    assert L.ita_mha_q8(ef._h, 0, xq.data_ptr(), yq.data_ptr(), 2, s) == -4
    assert L.ita_mha_long_q8(ef._h, 0, xq.data_ptr(), yq.data_ptr(), 1, 256, s) == -4
    assert L.ita_debug_encoder_stamps(ef._h, 0, x.data_ptr(), None, y.data_ptr(), 2, stamps.data_ptr(), s) == -4
    assert L.ita_debug_encoder_stamps(ef._h, 0, None, img.data_ptr(), y.data_ptr(), 2, stamps.data_ptr(), s) == -4
    assert L.ita_mha_f32(e8._h, 0, x.data_ptr(), y.data_ptr(), 2, s) == -4
    with pytest.raises(host.ITAError):
        ef.mha(x, 0, taps=True)
    # the drop-in symbol bound to a float layer reports through ita_last_error
    ef.bind_dispatch(0, host.DISPATCH_F32)
    buf = np.zeros(128 * 64, np.float32)
    out = np.zeros_like(buf)
    L.ITASelfAttention_workgroup(buf.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    assert L.ita_last_error() == -4
    e8.bind_dispatch(0, host.DISPATCH_F32)
    L.ITASelfAttention_workgroup(buf.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    assert L.ita_last_error() == 0
    ef.close(); e8.close()
    # E = 128: no float32 attention kernel
    with pytest.raises(host.ITAError, match="E = 64"):
        host.Engine(params.blob_from_float_params(synth.float_params(0, E=128)), device=0)
