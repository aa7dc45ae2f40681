"""The float graphs without the fusion tail on the MI355X: E = 128 (models/ITA_upsample_shuffle/model.py, two layers,
ita_attn_f32_kernel<128> + ita_ffn_f32_kernel<128>) and E = 64 (models/ITA_single_layer/model.py, one layer).
ita_mha_f32 against float64, ita_ffn_f32 and whole layers bit-equal to the oracle composition, the forward against the
reference fixtures (tests/golden/floatnt*) and FloatTwin in both tail modes, the serving forms against the eager
forward, and the refusals that remain at E = 128."""
import numpy as np
import pytest

from drone_oa_iree_vit_accelerator_amd import float_twin, host, params, synth
from gpu_support import cu
from float_graph_common import attn64, ln_like, repack, setup_notail as _setup, unpack

pytestmark = pytest.mark.gpu

def test_mha_f32_against_float64():
    """Bound: three times torch's own f32 error against float64 on the same frames, and never below 1e-5."""
    import torch
    d, fp, blob, L = _setup(128)
    eng = host.Engine(blob, device=0)
    twin = float_twin.FloatTwin(fp, num_layers=L)
    assert [eng.attn_kind(l) for l in range(L)] == [host.ATTN_F32] * L
    cases = [("tokens", d["s0.tok.out"])] + [(f"ln B={B}", ln_like(B, B, 128)) for B in (1, 3, 37, 1024)]
    for name, x in cases:
        B = x.shape[0]
        frames = np.arange(B) if B < 64 else np.random.RandomState(B).choice(B, 24, replace=False)
        for l in range(L):
            y = eng.mha_f32(cu(x), l).cpu().numpy()
            want = attn64(x[frames], fp, l)
            err = np.abs(y[frames] - want).max()
            terr = np.abs(twin._attention(torch.from_numpy(x[frames]), l).numpy() - want).max()
            assert err <= max(1e-5, 3 * terr), (name, l, err, terr)
            print(f"mha_f32 E=128 {name} layer {l}: |gpu - float64| = {err:.3e}, |torch f32 - float64| = {terr:.3e}")
    eng.close()


@pytest.mark.parametrize("E", [128, 64])
def test_ffn_f32_and_layer_bit_equal(oracle, E):
    _, _, blob, L = _setup(E)
    t = unpack(blob)
    eng = host.Engine(blob, device=0)
    for B in (1, 37):
        x = ln_like(B, 7 + B, E)
        x[0, 0, :8] = 0.0
        for l in range(L):
            hid = np.maximum(oracle.linear_f32(x, t[f"ffn{l}.w1f"], t[f"ffn{l}.b1f"]), np.float32(0))
            want = oracle.linear_f32(hid, t[f"ffn{l}.w2f"], t[f"ffn{l}.b2f"])
            assert np.array_equal(eng.ffn_f32(cu(x), l).cpu().numpy(), want), (B, l)
            att = eng.mha_f32(cu(x), l).cpu().numpy()
            x1 = oracle.add_ln(x, att, t[f"norm1_{l}.w"], t[f"norm1_{l}.b"])
            hid = np.maximum(oracle.linear_f32(x1, t[f"ffn{l}.w1f"], t[f"ffn{l}.b1f"]), np.float32(0))
            want = oracle.add_ln(x1, oracle.linear_f32(hid, t[f"ffn{l}.w2f"], t[f"ffn{l}.b2f"]), t[f"norm2_{l}.w"], t[f"norm2_{l}.b"])
            assert np.array_equal(eng.encoder_layer(cu(x), l).cpu().numpy(), want), (B, l)
    eng.close()


@pytest.mark.parametrize("E", [128, 64])
def test_layers_from_reference_tokens(E):
    d, _, blob, L = _setup(E)
    eng = host.Engine(blob, device=0)
    x = cu(d["s0.tok.out"])
    for l in range(L):
        x = eng.encoder_layer(x, l)
        err = np.abs(x.cpu().numpy() - d[f"s0.x2_{l}"]).max()
        assert err <= 2e-5, (l, err)
    eng.close()


@pytest.mark.parametrize("E", [128, 64])
def test_forward_against_reference_and_float_twin(E):
    import torch
    d, fp, blob, L = _setup(E)
    eng = host.Engine(blob, device=0)
    twin = float_twin.FloatTwin(fp, num_layers=L)
    fr = synth.frames(70 + E, 64)
    tv0, tst0, ttp = twin.forward(fr["img_u8"], fr["desvel"], fr["quat"], taps=True)
    rs = np.random.RandomState(E)
    hid = tuple((0.1 * rs.standard_normal((3, 64, 128))).astype(np.float32) for _ in range(2))
    tv1, tst1 = twin.forward(fr["img_u8"], fr["desvel"], fr["quat"], hidden=hid)
    for mode in (0, 1):
        eng.set_tail_mode(mode)
        v0, st, tp = eng.forward(cu(d["in0.img_u8"]), cu(d["in0.desvel"]), cu(d["in0.quat"]), taps=True)
        v1, st1 = eng.forward(cu(d["in1.img_u8"]), cu(d["in1.desvel"]), cu(d["in1.quat"]), st)
        torch.cuda.synchronize()
        assert np.abs(tp["tokens"].cpu().numpy() - d["s0.tok.out"]).max() <= 2e-5
        for k, w in (("x1", f"x1_{L - 1}"), ("x2", f"x2_{L - 1}")) + ((("dec", "dec"),) if mode == 0 else ()):
            err = np.abs(tp[k].cpu().numpy() - d["s0." + w]).max()
            assert err <= 1e-4, (mode, k, err)
        for g, k in ((v0, "s0.vel"), (st[0], "s0.h"), (st[1], "s0.c"), (v1, "s1.vel"), (st1[0], "s1.h"), (st1[1], "s1.c")):
            err = np.abs(g.cpu().numpy() - d[k]).max()
            assert err <= 5e-4, (mode, k, err)
        g0, gst, gtp = eng.forward(cu(fr["img_u8"]), cu(fr["desvel"]), cu(fr["quat"]), taps=True)
        g1, gst1 = eng.forward(cu(fr["img_u8"]), cu(fr["desvel"]), cu(fr["quat"]), (cu(hid[0]), cu(hid[1])))
        assert np.abs(gtp["tokens"].cpu().numpy() - ttp["tokens"].numpy()).max() <= 2e-5
        for k in ("x1", "x2") + (("dec",) if mode == 0 else ()):
            err = np.abs(gtp[k].cpu().numpy() - ttp[k].numpy()).max()
            assert err <= 1e-4, (mode, k, err)
        for g, w in ((g0, tv0), (gst[0], tst0[0]), (gst[1], tst0[1]), (g1, tv1), (gst1[0], tst1[0]), (gst1[1], tst1[1])):
            assert np.abs(g.cpu().numpy() - w.numpy()).max() <= 5e-4
    eng.close()


def test_frames_independent_runs_repeatable_in_place():
    _, _, blob, _ = _setup(128)
    eng = host.Engine(blob, device=0)
    x = ln_like(37, 5, 128)
    y = eng.mha_f32(cu(x), 1).cpu().numpy()
    assert np.array_equal(eng.mha_f32(cu(x), 1).cpu().numpy(), y)
    z = eng.encoder_layer(cu(x), 1).cpu().numpy()
    assert np.array_equal(eng.encoder_layer(cu(x), 1).cpu().numpy(), z)
    for b in (0, 17, 36):
        assert np.array_equal(eng.mha_f32(cu(x[b:b + 1]), 1).cpu().numpy()[0], y[b]), b
        assert np.array_equal(eng.encoder_layer(cu(x[b:b + 1]), 1).cpu().numpy()[0], z[b]), b
        assert np.array_equal(eng.mha_f32(cu(np.concatenate([x[b:b + 1], x[:3]])), 1).cpu().numpy()[0], y[b]), b
    xx = cu(x)
    host.lib().ita_encoder_layer(eng._h, 1, xx.data_ptr(), xx.data_ptr(), 37, host._stream_ptr(eng.device))
    assert np.array_equal(xx.cpu().numpy(), z)
    eng.close()


def test_serving_forms_and_profiler():
    import torch
    _, _, blob, _ = _setup(128)
    eng = host.Engine(blob, device=0)
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
    g = eng.graphed_step(B)
    st = (torch.zeros((3, B, 128), device="cuda"), torch.zeros((3, B, 128), device="cuda"))
    for t in range(T):
        g.img.copy_(cu(frames[t]["img_u8"])); g.desvel.copy_(cu(frames[t]["desvel"]).reshape(B)); g.quat.copy_(cu(frames[t]["quat"]))
        vg = g().clone()
        ve, st = eng.forward(cu(frames[t]["img_u8"]), cu(frames[t]["desvel"]), cu(frames[t]["quat"]), st)
        assert torch.equal(vg, ve) and torch.equal(g.h, st[0]) and torch.equal(g.c, st[1]), t
    del g
    fr = synth.frames(3, 8)
    eng.profile_begin(4)
    for _ in range(3):
        eng.forward(cu(fr["img_u8"]), cu(fr["desvel"]), cu(fr["quat"]))
    ms, n = eng.profile_end()
    assert n == 3 and ms["mha"] > 0 and ms["ffn"] > 0
    eng.close()


@pytest.mark.parametrize("stages", [2, 3])
def test_pipelined_steps_equal_sequential_forward(stages):
    import torch
    _, _, blob, _ = _setup(128)
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


def test_refusals_at_e128():
    import torch
    _, _, blob, _ = _setup(128)
    with pytest.raises(host.ITAError, match="E = 64"):   # a float fusion tail exists only at E = 64
        host.Engine(params.blob_from_float_params(synth.float_params(0, E=128, num_layers=2), 2), device=0)
    with pytest.raises(host.ITAError, match="E = 64"):   # no ITAW0002 (int8 attention, float FFN) graph at E = 128
        host.Engine(repack(blob, unpack(blob), magic=b"ITAW0002"), device=0)
    eng = host.Engine(blob, device=0)
    L = host.lib()
    x = cu(ln_like(2, 1, 128))
    y = torch.empty_like(x)
    xq = torch.zeros((2, 128, 128), dtype=torch.int8, device="cuda")
    yq = torch.empty_like(xq)
    s = host._stream_ptr(0)
    assert L.ita_mha_int8(eng._h, 0, x.data_ptr(), y.data_ptr(), 2, s) == -4
    assert L.ita_mha_q8(eng._h, 0, xq.data_ptr(), yq.data_ptr(), 2, s) == -4
    assert L.ita_mha_long_q8(eng._h, 0, xq.data_ptr(), yq.data_ptr(), 1, 256, s) == -4
    eng.close()
