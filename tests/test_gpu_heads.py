"""Multi-head int8 attention on the GPU (ita_mha_kernel<E, H>, H = 2, 3, 4, 6): a blob whose header says H > 1 loads, runs
the two-launch block route behind the stand-alone tokenizer, and computes the numpy definition (mha_heads_ref) bit for
bit -- every tap, the block output, the encoder layer, the whole forward in both tail modes and the sequence form.  The
entry points that need a stream-kernel image refuse such a blob before launching anything."""
import functools

import numpy as np
import pytest

import heads_common as hc
from conftest import golden_files
from drone_oa_iree_vit_accelerator_amd import host, mha_heads_ref, params, synth
from gpu_support import cu

pytestmark = pytest.mark.gpu

FIX = hc.FIX_HEADS + hc.FIX_HEADS_2L
TAPS = ("x_q", "Q", "K", "V", "logits", "probs", "ctx", "out_q")
UNSUPPORTED = "ita status -4:"


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@functools.lru_cache(maxsize=None)
def _block_case(path):
    """five distinct block inputs (the fixture's, and the tokens of four synthetic frames) with the numpy definition of
    the attention block and the composed encoder layer on them; computed once, read-only"""
    from oracle import oracle
    oracle.build()
    d, H, E, nl, t, fp, blob = hc.case(path)
    tok = oracle.tokenizer(synth.frames(7, 4)["img_u8"], fp["tokenizer.conv.weight"], fp["tokenizer.conv.bias"],
                           fp["tokenizer.norm.weight"], fp["tokenizer.norm.bias"])
    x = np.concatenate([d["s0.tok.out"][:1], tok]).astype(np.float32)   # (layer 0's block input is the token tensor)
    y, taps = mha_heads_ref.mha(x, t, H)
    x1, x2 = hc.encoder_layer(oracle, x, t, fp, H)
    return x, y, taps, x1, x2


@pytest.mark.parametrize("path", FIX, ids=hc.fixture_id)
def test_attention_block_equals_the_definition(torch_cuda, path):
    """B = 1, 3 and CU count + 3 (the grid-stride loop reuses a workgroup's LDS for a second frame)"""
    torch = torch_cuda
    d, H, E, nl, t, fp, blob = hc.case(path)
    x, y, taps, x1, x2 = _block_case(path)
    eng = host.Engine(blob, device=0)
    assert (eng.H, eng.E) == (H, E)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for B in (1, 3, cus + 3):
        idx = np.arange(B) % len(x)
        xb = cu(x[idx])
        gy, gt = eng.mha(xb, taps=True)
        assert tuple(gt["logits"].shape) == (B, H, 128, 128) and tuple(gt["probs"].shape) == (B, H, 128, 128)
        for k in TAPS:
            np.testing.assert_array_equal(gt[k].cpu().numpy(), taps[k][idx], err_msg=f"{k} B={B}")
        np.testing.assert_array_equal(gy.cpu().numpy(), y[idx], err_msg=f"B={B}")
        np.testing.assert_array_equal(eng.mha(xb).cpu().numpy(), y[idx], err_msg=f"no taps, B={B}")
        np.testing.assert_array_equal(eng.encoder_layer(xb).cpu().numpy(), x2[idx], err_msg=f"encoder layer, B={B}")
    # the reference's own tensors: the fixture has no near-tie logit (tests/test_heads_cpu.py), so all of them
    if "s0.attn0.probs.in" in d:
        np.testing.assert_array_equal(taps["logits"][:1], d["s0.attn0.probs.in"][:1])
    np.testing.assert_array_equal(taps["out_q"][:1], d["s0.attn0.out_q"][:1])
    eng.close()


def test_crafted_heads_do_not_leak(torch_cuda):
    """H = 4 (head width 48: one 16x16x64 step with a zero fragment): head 1 with zero Q, so that all its logits are equal
    and every probability is 1 (sum 32768, inv 510, (256 * 510) >> 16 = 1) whatever K holds; head 2 with saturated K
    codes.  A fragment past the head's range that is not zero, or a head reading a neighbour's chunks, changes head 1."""
    torch = torch_cuda
    d, H, E, nl, t, fp, blob = hc.case([p for p in hc.FIX_HEADS if hc.heads_of(p) == 4][0])
    t = {k: v.copy() for k, v in t.items()}
    hd = 192 // H
    t["attn0.wq"][hd:2 * hd] = 0
    t["attn0.bq"][hd:2 * hd] = 0
    t["attn0.wk"][2 * hd:3 * hd] = 0
    t["attn0.bk"][2 * hd:3 * hd] = np.where(np.arange(hd) % 2 == 0, 1 << 24, -(1 << 24)).astype(np.int32)
    blob = params.pack_blob(t, E=64, H=H, has_tail=False)
    x = _block_case(hc.FIX_HEADS[0])[0][:3]
    y, taps = mha_heads_ref.mha(x, t, H)
    assert (taps["Q"][..., hd:2 * hd] == 0).all() and (taps["probs"][:, 1] == 1).all()
    k2 = taps["K"][..., 2 * hd:3 * hd]
    assert (k2[..., 0::2] == 127).all() and (k2[..., 1::2] == -128).all()
    assert len(np.unique(taps["probs"][:, 0])) > 2 and len(np.unique(taps["probs"][:, 3])) > 2   # the other heads: real rows
    eng = host.Engine(blob, device=0)
    gy, gt = eng.mha(cu(x), taps=True)
    assert (gt["probs"][:, 1] == 1).all().item()
    for k in TAPS:
        np.testing.assert_array_equal(gt[k].cpu().numpy(), taps[k], err_msg=k)
    np.testing.assert_array_equal(gy.cpu().numpy(), y)
    eng.close()


GRAPHS = hc.FIX_GRAPHS


@pytest.mark.parametrize("path", GRAPHS, ids=hc.fixture_id)
def test_whole_forward_two_steps_and_sequence(torch_cuda, oracle, path):
    """u8 and f32 frames, two time steps with carried state: tail mode 0 equal to the composed oracle, tail mode 1 within
    2e-5 (the suite's bound for the split-precision tail); forward_sequence (T = 3, B = 2) equal to three forward calls"""
    torch = torch_cuda
    d, H, E, nl, t, fp, blob = hc.case(path)
    eng = host.Engine(blob, device=0, reserve=6)
    fr = [synth.frames(40 + s, 2) for s in range(3)]
    for f32 in (False, True):
        imgs = [f["img_u8"].astype(np.float32) / np.float32(255.0) if f32 else f["img_u8"] for f in fr]
        o0 = hc.forward(oracle, imgs[0], t, fp, nl, H, fr[0]["desvel"], fr[0]["quat"])
        for mode in (0, 1):
            eng.set_tail_mode(mode)
            v0, st0 = eng.forward(cu(imgs[0]), cu(fr[0]["desvel"]), cu(fr[0]["quat"]))
            v1, st1 = eng.forward(cu(imgs[1]), cu(fr[1]["desvel"]), cu(fr[1]["quat"]), st0)
            got = (v0, st0[0], st0[1], v1, st1[0], st1[1])
            # the second step from the state the engine carried (in mode 0 that is the oracle's own, bit for bit)
            o1 = hc.forward(oracle, imgs[1], t, fp, nl, H, fr[1]["desvel"], fr[1]["quat"], st0[0].cpu().numpy(), st0[1].cpu().numpy())
            for name, g, w in zip(("vel0", "h0", "c0", "vel1", "h1", "c1"), got, o0 + o1):
                g = g.cpu().numpy()
                print(f"{hc.fixture_id(path)} f32={f32} mode {mode}: max |{name} - oracle| = {np.abs(g - w).max():.3e}")
                if mode == 0:
                    np.testing.assert_array_equal(g, w, err_msg=f"{name} f32={f32}")
                else:
                    np.testing.assert_allclose(g, w, atol=2e-5, rtol=0, err_msg=f"{name} f32={f32}")
    # against the reference's own outputs, from its image: the suite's end-to-end bound on the velocity
    eng.set_tail_mode(1)
    v, _ = eng.forward(cu(d["in0.img_u8"]), cu(d["in0.desvel"]), cu(d["in0.quat"]))
    np.testing.assert_allclose(v.cpu().numpy(), d["s0.vel"], atol=5e-4, rtol=0)
    # the sequence form and the encoder's taps
    img = np.stack([f["img_u8"] for f in fr]); dv = np.stack([f["desvel"].reshape(2) for f in fr]); qt = np.stack([f["quat"] for f in fr])
    rs = np.random.RandomState(1)
    h0, c0 = ((0.3 * rs.standard_normal((3, 2, 128))).astype(np.float32) for _ in range(2))
    st, vels = (cu(h0), cu(c0)), []
    for s in range(3):
        vs, st = eng.forward(cu(img[s]), cu(dv[s]), cu(qt[s]), st)
        vels.append(vs)
    sv, (sh, sc) = eng.forward_sequence(cu(img), cu(dv), cu(qt), (cu(h0), cu(c0)))
    torch.cuda.synchronize()
    assert eng.head_status() == 0
    assert torch.equal(sv, torch.stack(vels)) and torch.equal(sh, st[0]) and torch.equal(sc, st[1])
    _, _, tp = eng.forward(cu(img[0]), cu(dv[0]), cu(qt[0]), taps=True)
    tok = oracle.tokenizer(img[0], fp["tokenizer.conv.weight"], fp["tokenizer.conv.bias"], fp["tokenizer.norm.weight"],
                           fp["tokenizer.norm.bias"])
    np.testing.assert_array_equal(tp["tokens"].cpu().numpy(), tok)
    # x1 is the last layer's attention launch with the residual and LayerNorm1 fused (fuse_ln = 1), the launch this route
    # makes; x2 the FFN launch behind it
    x1, x2 = hc.encoder(oracle, tok, t, fp, nl, H)
    np.testing.assert_array_equal(tp["x1"].cpu().numpy(), x1)
    np.testing.assert_array_equal(tp["x2"].cpu().numpy(), x2)
    # the same two taps beyond one frame per workgroup, from f32 frames: five distinct frames, tiled
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    f5 = synth.frames(45, 5)
    img5 = f5["img_u8"].astype(np.float32) / np.float32(255.0)
    tok5 = oracle.tokenizer(img5, fp["tokenizer.conv.weight"], fp["tokenizer.conv.bias"], fp["tokenizer.norm.weight"],
                            fp["tokenizer.norm.bias"])
    x1, x2 = hc.encoder(oracle, tok5, t, fp, nl, H)
    idx = np.arange(cus + 3) % 5
    eng.close()
    eng = host.Engine(blob, device=0)      # (the first engine's workspace is pinned at six frames)
    _, _, tp = eng.forward(cu(img5[idx]), cu(f5["desvel"][idx]), cu(f5["quat"][idx]), taps=True)
    np.testing.assert_array_equal(tp["x1"].cpu().numpy(), x1[idx])
    np.testing.assert_array_equal(tp["x2"].cpu().numpy(), x2[idx])
    eng.close()


def test_split_forms_equal_forward(torch_cuda):
    """tail, front / back, encode / fold / back and the pipelined form on an H = 3 blob: the bits of forward"""
    torch = torch_cuda
    d, H, E, nl, t, fp, blob = hc.case(GRAPHS[0])
    B, T = 3, 2
    eng = host.Engine(blob, device=0, reserve=B)
    fr = [synth.frames(60 + s, B) for s in range(T)]
    zero = lambda: (torch.zeros((3, B, 128), device="cuda"), torch.zeros((3, B, 128), device="cuda"))
    ref, st = [], zero()
    for f in fr:
        v, st = eng.forward(cu(f["img_u8"]), cu(f["desvel"]), cu(f["quat"]), st)
        ref.append((v.clone(), st[0].clone(), st[1].clone()))
    _, _, tp = eng.forward(cu(fr[0]["img_u8"]), cu(fr[0]["desvel"]), cu(fr[0]["quat"]), taps=True)
    vt, (ht, ct) = eng.tail(tp["x2"], cu(fr[0]["desvel"]), cu(fr[0]["quat"]))
    assert torch.equal(vt, ref[0][0]) and torch.equal(ht, ref[0][1]) and torch.equal(ct, ref[0][2])
    for split in (False, True):
        st = zero()
        for s, f in enumerate(fr):
            if split:
                eng.encode(cu(f["img_u8"]), 0)
                eng.fold(B, 0, 0)
            else:
                eng.front(cu(f["img_u8"]), 0)
            out = (torch.empty((B, 3), device="cuda"), *zero())
            eng.back(cu(f["desvel"]).reshape(B), cu(f["quat"]), st, out, 0)
            torch.cuda.synchronize()
            assert all(torch.equal(a, b) for a, b in zip(out, ref[s])), (split, s)
            st = out[1:]
    h, c = zero()
    vels = [torch.empty((B, 3), device="cuda") for _ in range(T)]
    sf, sb = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    eng.pipelined([cu(f["img_u8"]) for f in fr], [cu(f["desvel"]).reshape(B) for f in fr], [cu(f["quat"]) for f in fr],
                  (h, c), vels, sf, sb)
    torch.cuda.synchronize()
    assert all(torch.equal(vels[s], ref[s][0]) for s in range(T)) and torch.equal(h, ref[-1][1]) and torch.equal(c, ref[-1][2])
    assert eng.head_status() == 0
    eng.close()


def test_dropin_symbol_runs_the_heads(torch_cuda):
    """ITASelfAttention_workgroup (host buffers of 1 x 128 x 128 f32) bound to a layer of the E = 128, H = 4 blob"""
    import ctypes
    d, H, E, nl, t, fp, blob = hc.case(hc.FIX_HEADS_2L[0])
    x, y, *_ = _block_case(hc.FIX_HEADS_2L[0])
    eng = host.Engine(blob, device=0)
    eng.bind_dispatch(0, host.DISPATCH_F32)
    xin, out = x[1].copy(), np.empty_like(x[1])
    lib = host.lib()
    lib.ITASelfAttention_workgroup(xin.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p))
    assert lib.ita_last_error() == 0, lib.ita_error_string()
    np.testing.assert_array_equal(out, y[1])
    eng.close()


def test_refusals_and_reload(torch_cuda, oracle):
    """what needs a stream-kernel image refuses an H > 1 blob with ITA_ERR_UNSUPPORTED before any launch; blobs the
    kernels are not built for do not load; the handle then takes an H = 1 blob and runs the stream kernel as before"""
    torch = torch_cuda
    d, H, E, nl, t, fp, blob = hc.case(GRAPHS[0])
    eng = host.Engine(blob, device=0)
    xq = torch.zeros((2, 128, 64), dtype=torch.int8, device="cuda")
    with pytest.raises(host.ITAError, match=UNSUPPORTED):
        eng.mha_q8(xq)
    with pytest.raises(host.ITAError, match=UNSUPPORTED):
        eng.encoder_stamps(torch.zeros((2, 128, 64), device="cuda"))
    fr = synth.frames(3, 2)
    sh, sc = torch.zeros((3, 4, 128), device="cuda"), torch.zeros((3, 4, 128), device="cuda")
    with pytest.raises(host.ITAError, match=UNSUPPORTED):
        eng.forward_slots(cu(fr["img_u8"]), cu(fr["desvel"]), cu(fr["quat"]), sh, sc, torch.tensor([2, 0], device="cuda"))
    torch.cuda.synchronize()
    assert float(sh.abs().max()) == 0.0 and float(sc.abs().max()) == 0.0        # nothing ran
    # (the long-sequence entry refuses E = 64 before it looks at the image, so its head-count refusal can only be reached
    #  on an E = 128 blob: the H = 4 one)
    e128 = host.Engine(hc.case(hc.FIX_HEADS_2L[0])[6], device=0)
    with pytest.raises(host.ITAError, match=UNSUPPORTED):
        e128.mha_long_q8(torch.zeros((1, 256, 128), dtype=torch.int8, device="cuda"))
    e128.close()
    # the handle still runs after the refusals
    x, y, *_ = _block_case(GRAPHS[0])
    np.testing.assert_array_equal(eng.mha(cu(x[:2])).cpu().numpy(), y[:2])
    # loads that stay refused: the float graph with two heads, a head count the kernel is not built for, and the
    # attention-only graph (int8 attention, float FFN) with more than one head
    set_h = lambda b, h: b[:28] + np.int32(h).tobytes() + b[32:]
    fblob = params.blob_from_float_params(synth.float_params(0, E=64))
    oa = params.load_fixture(golden_files("onlyattn1l_E64_s0_B2.npz")[0])
    oblob = params.blob_from_record(oa, synth.float_params(0, E=64), E=64)
    assert fblob[:8] == params.MAGIC_F32 and oblob[:8] == params.MAGIC_FFN_F32
    for bad in (set_h(fblob, 2), set_h(blob, 5), set_h(oblob, 2)):
        with pytest.raises(host.ITAError, match=UNSUPPORTED):
            eng.load_weights(bad)
    # the same handle with an H = 1 blob: the stream kernel, equal to the oracle
    d1 = params.load_fixture(golden_files("vitlstm_E64_seed0_B2.npz")[0])
    blob1 = params.blob_from_record(d1, fp, E=64)
    eng.load_weights(blob1)
    assert eng.H == 1
    t1 = params.attention_tensors(d1, "attn0.", 0)
    x1 = d1["s0.attn0.x_q.in"]
    want, wt = oracle.mha(x1, t1, taps=True)
    np.testing.assert_array_equal(eng.mha(cu(x1)).cpu().numpy(), want)
    np.testing.assert_array_equal(eng.mha_q8(cu(wt["x_q"])).cpu().numpy(), wt["out_q"])      # needs the stream image
    gy, gt = eng.mha(cu(x1), taps=True)
    assert tuple(gt["logits"].shape) == (2, 128, 128)
    np.testing.assert_array_equal(gt["probs"].cpu().numpy(), wt["probs"])
    vel, (h, c) = eng.forward(cu(d1["in0.img_u8"]), cu(d1["in0.desvel"]), cu(d1["in0.quat"]))
    ovel, oh, oc = oracle.forward(blob1, d1["in0.img_u8"], d1["in0.desvel"], d1["in0.quat"])
    np.testing.assert_allclose(vel.cpu().numpy(), ovel, atol=2e-5, rtol=0)
    np.testing.assert_allclose(h.cpu().numpy(), oh, atol=2e-5, rtol=0)
    eng.close()
