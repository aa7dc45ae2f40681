"""The float graph on long sequences on the MI355X: ita_mha_long_f32 (Engine.mha_long_f32) against a float64 restatement
of ITASelfAttention.forward over rows of S keys, ita_encoder_layer_long_f32 (Engine.encoder_layer_long_f32 /
encode_long_f32 / encode_frames_long_f32) against the float64 layer on ITAW0003 blobs and, bit for bit, against the oracle
composition on ITAW0002 blobs, and the refusals of the two entries.

Bound (tests/long_f32_common.py: bound): the project's rule of test_mha_f32_against_float64, max(1e-5, 3 x e_torch), with
e_torch the error of torch's CPU f32 attention (or layer) against the same float64 restatement on the same rows.  The error
is set by the f32 rounding of q, k and of logits of magnitude 100 .. 400, which exp amplifies, not by the order of the keys:
a numpy f32 emulation of the running-maximum algorithm with 64-key tiles lies within 1 % of e_torch on every case here, and
the same emulation WITHOUT the rescale of the context accumulators is off by 1.4 .. 5.7 on every input kind and shape.
Measured on an MI355X, err / e_torch: 0.16 .. 0.64 on the plain and ramped rows, 0.20 .. 1.87 with one dominant key,
0.17 .. 0.57 for the whole layer.

Shapes (S, B): (128, 3) one query tile, two 64-key units; (256, 2) / (384, 2) even and odd tile counts, B > 1 the frame
strides of the workspace; (1024, 1) a longer sum.  E = 64 (one layer) and E = 128 (two layers, both tested)."""
import numpy as np
import pytest

from conftest import golden_files
from drone_oa_iree_vit_accelerator_amd import host, params, synth
from gpu_support import cu, engine_pool
import long_f32_common as lc
from long_f32_common import SHAPES, LAYERS
from long_cases import long_f32 as quantiser_safe_tokens
from only_attn_common import fp as only_attn_fp, tensors as only_attn_tensors

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0


@pytest.fixture(scope="module")
def engines():
    yield from engine_pool(lambda E: lc.case(E)[1])


def _check(got, want, e_torch, what):
    """prints (err, e_torch), then asserts: every output finite, err within the rule's bound"""
    assert np.isfinite(got).all(), what
    err = float(np.abs(got - want).max())
    print(f"{what}: |gpu - float64| = {err:.3e}, |torch f32 - float64| = {e_torch:.3e}, ratio {err / e_torch:.2f}")
    assert err <= lc.bound(e_torch), (what, err, e_torch)
    return err


# ---- 1, 2: mha_long_f32 against float64
@pytest.mark.parametrize("S,B", SHAPES)
@pytest.mark.parametrize("E", [64, 128])
@pytest.mark.parametrize("kind", ["plain", "ramp", "ramp_rev"])
def test_mha_long_f32_against_float64(engines, kind, E, S, B):
    eng = engines(E)
    assert [eng.attn_kind(l) for l in range(LAYERS[E])] == [host.ATTN_F32] * LAYERS[E]
    x = cu(lc.inputs(kind, E, S, B))
    for l in range(LAYERS[E]):
        want, e_torch = lc.attn_ref(kind, E, S, B, l)
        _check(eng.mha_long_f32(x, l).cpu().numpy(), want, e_torch, f"mha_long_f32 {kind} E={E} S={S} B={B} layer {l}")


@pytest.mark.parametrize("S,B", SHAPES)
@pytest.mark.parametrize("E", [64, 128])
@pytest.mark.parametrize("kind", ["spike_last", "spike_first"])
def test_mha_long_f32_one_dominant_key(engines, kind, E, S, B):
    """one token of 4 x the norm in the last / first key tile: the rule's bound, and the rows that are one-hot on it in
    float64 (probability > 1 - 1e-6) lie within that bound of out_proj(v of that token).

    Measured on an MI355X: err / e_torch 0.20 .. 1.87 over the 24 (kind, E, S, B, layer) cases.  (With Q, K and the
    logits summed as one fmaf chain each, the kernel's first form, it was 0.72 .. 3.22 and spike_last, E = 128, S = 256,
    layer 1 missed the bound: the block sums of ita_long_f32_kernel.h are there for this test.)"""
    eng = engines(E)
    fp = lc.case(E)[0]
    xn = lc.inputs(kind, E, S, B)
    pos = S - 1 if kind == "spike_last" else 0
    for l in range(LAYERS[E]):
        want, e_torch = lc.attn_ref(kind, E, S, B, l)
        got = eng.mha_long_f32(cu(xn), l).cpu().numpy()
        _check(got, want, e_torch, f"mha_long_f32 {kind} E={E} S={S} B={B} layer {l}")
        p, v = lc.probs64(xn, fp, l)
        onehot = p[:, :, pos] > 1.0 - 1e-6
        assert onehot.sum() >= S // 8, (kind, l, int(onehot.sum()))
        vdom = lc.out_proj64(v[:, pos], fp, l)                     # (B, E)
        d = np.abs(got - vdom[:, None, :])[onehot].max()
        assert d <= lc.bound(e_torch), (kind, l, d, e_torch)


# ---- 3: repeatability
@pytest.mark.parametrize("E", [64, 128])
def test_runs_repeatable_and_frames_independent(engines, E):
    import torch
    eng = engines(E)
    for S, B in ((256, 2), (384, 2), (128, 3)):
        x = cu(lc.inputs("ramp", E, S, B))
        y = eng.mha_long_f32(x)
        assert torch.equal(y, eng.mha_long_f32(x)), (S, B)
        assert torch.equal(eng.mha_long_f32(x.flip(0).contiguous()).flip(0), y), (S, B)
        for b in range(B):
            assert torch.equal(eng.mha_long_f32(x[b:b + 1].contiguous())[0], y[b]), (S, B, b)
        z = eng.encoder_layer_long_f32(x)
        assert torch.equal(z, eng.encoder_layer_long_f32(x)), (S, B)
        assert torch.equal(eng.encoder_layer_long_f32(x[B - 1:].contiguous())[0], z[B - 1]), (S, B)


# ---- 4: duplicated sequence
@pytest.mark.parametrize("S,B", [(128, 3), (384, 2)])
@pytest.mark.parametrize("E", [64, 128])
@pytest.mark.parametrize("kind", ["plain", "ramp"])
def test_duplicated_sequence(engines, kind, E, S, B):
    """cat(x, x) along the sequence: rows S .. 2S - 1 see the same query and the same keys in the same order as rows
    0 .. S - 1 (bit-equal), and softmax over the doubled keys is the softmax over S keys: both halves within the rule's
    bound of the S-length float64 result"""
    import torch
    eng = engines(E)
    x = cu(lc.inputs(kind, E, S, B))
    xx = torch.cat([x, x], dim=1).contiguous()
    for l in range(LAYERS[E]):
        y = eng.mha_long_f32(xx, l)
        assert torch.equal(y[:, :S], y[:, S:]), (kind, E, S, l)
        want, e_torch = lc.attn_ref(kind, E, S, B, l)
        _check(y[:, S:].cpu().numpy(), want, e_torch, f"cat(x, x) {kind} E={E} S={S} B={B} layer {l}")


# ---- 5: S = 128 against mha_f32
@pytest.mark.parametrize("E", [64, 128])
def test_one_tile_beside_mha_f32(engines, E):
    """no bit-equality (the summation order differs): both within the bound of float64 on the same rows"""
    eng = engines(E)
    for kind in ("plain", "ramp"):
        x = cu(lc.inputs(kind, E, 128, 3))
        for l in range(LAYERS[E]):
            want, e_torch = lc.attn_ref(kind, E, 128, 3, l)
            _check(eng.mha_long_f32(x, l).cpu().numpy(), want, e_torch, f"mha_long_f32 {kind} E={E} S=128 layer {l}")
            _check(eng.mha_f32(x, l).cpu().numpy(), want, e_torch, f"mha_f32      {kind} E={E} S=128 layer {l}")


# ---- 6: the float layer
@pytest.mark.parametrize("S,B", SHAPES)
@pytest.mark.parametrize("E", [64, 128])
def test_encoder_layer_long_f32_against_float64(engines, E, S, B):
    """LN2(x1 + ffn(x1)), x1 = LN1(x + attn(x)) against float64, bound from the same composition in torch f32 on the CPU;
    out aliasing x gives the bit-identical result"""
    import torch
    eng = engines(E)
    for kind in ("plain", "ramp"):
        x = cu(lc.inputs(kind, E, S, B))
        for l in range(LAYERS[E]):
            want, e_torch = lc.layer_ref(kind, E, S, B, l)
            got = eng.encoder_layer_long_f32(x, l)
            _check(got.cpu().numpy(), want, e_torch, f"encoder_layer_long_f32 {kind} E={E} S={S} B={B} layer {l}")
            alias = x.clone()
            assert eng.encoder_layer_long_f32(alias, l, out=alias) is alias
            assert torch.equal(alias, got), f"E={E} S={S} layer {l}: out aliasing x"


def test_encode_long_f32_is_the_layers_chained(engines):
    import torch
    eng = engines(128)
    assert eng.num_layers == 2
    x = cu(lc.inputs("ramp", 128, 384, 2))
    keep = x.clone()
    got = eng.encode_long_f32(x)
    assert torch.equal(x, keep), "encode_long_f32 changed its input"
    assert torch.equal(got, eng.encoder_layer_long_f32(eng.encoder_layer_long_f32(x, 0), 1))
    assert bool(torch.isfinite(got).all())


# ---- 7: the attention-only QAT graph (ITAW0002), by equality
@pytest.mark.parametrize("S,B", SHAPES)
@pytest.mark.parametrize("fixture", ["onlyattn1l_E64_s0_B2", "onlyattn2l_E64_s1_B2"])
def test_encoder_layer_long_f32_only_attn_equals_oracle(oracle, fixture, S, B):
    """int8 long attention + LN1, float FFN + LN2: every kernel of the route has a bit-exact definition -- the oracle
    composition of tests/test_gpu_only_attn.py; at S = 128 also Engine.encoder_layer; out aliasing x"""
    import torch
    d = params.load_fixture(golden_files(fixture + ".npz")[0])
    fp = only_attn_fp(d)
    L = int(d["meta.num_layers"])
    t = only_attn_tensors(d, fp)
    eng = host.Engine(params.blob_from_record(d, fp, E=64, num_layers=L), device=0)
    for l in range(L):
        assert eng.ffn_kind(l) == host.FFN_F32 and eng.attn_kind(l) == host.ATTN_INT8
        x = quantiser_safe_tokens(S + B + l, B, S, 64, t, l)
        xc = cu(x)
        got = eng.encoder_layer_long_f32(xc, l)
        x1 = oracle.add_ln(x, oracle.mha(x, t, l), t[f"norm1_{l}.w"], t[f"norm1_{l}.b"])
        hid = np.maximum(oracle.linear_f32(x1, t[f"ffn{l}.w1f"], t[f"ffn{l}.b1f"]), np.float32(0))
        want = oracle.add_ln(x1, oracle.linear_f32(hid, t[f"ffn{l}.w2f"], t[f"ffn{l}.b2f"]), t[f"norm2_{l}.w"], t[f"norm2_{l}.b"])
        np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=f"{fixture} layer {l}")
        if S == 128:
            assert torch.equal(eng.encoder_layer(xc, l), got), f"{fixture} layer {l}"
        alias = xc.clone()
        assert eng.encoder_layer_long_f32(alias, l, out=alias) is alias
        assert torch.equal(alias, got), f"{fixture} layer {l}: out aliasing x"
    eng.close()


# ---- 8: refusals
def _status(eng, entry, seq_len=256):
    """the entry's status on a (1, 256, E) buffer pair declared as seq_len long; the sentinel-filled output must stay"""
    import torch
    out = torch.full((1, 256, eng.E), SENTINEL, dtype=torch.float32, device="cuda")
    x = torch.zeros_like(out)
    rc = getattr(host.lib(), entry)(eng._h, 0, x.data_ptr(), out.data_ptr(), 1, seq_len, host._stream_ptr(eng.device))
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()), f"{entry}: a refused call wrote to its output"
    return rc


def test_refusals_before_any_launch(engines):
    fx = params.load_fixture(golden_files("vitlstm_E64_seed0_B2.npz")[0])
    e1 = host.Engine(params.blob_from_record(fx, synth.float_params(0, E=64), E=64), device=0)          # ITAW0001
    d = params.load_fixture(golden_files("onlyattn1l_E64_s0_B2.npz")[0])
    e2 = host.Engine(params.blob_from_record(d, only_attn_fp(d), E=64, num_layers=1), device=0)        # ITAW0002
    assert _status(e1, "ita_mha_long_f32") == -4
    assert "ita_mha_long_int8" in host.lib().ita_error_string().decode()
    assert _status(e2, "ita_mha_long_f32") == -4
    assert _status(e1, "ita_encoder_layer_long_f32") == -4
    assert "ita_encoder_layer_long" in host.lib().ita_error_string().decode()
    e1.close(); e2.close()
    for E in (64, 128):
        eng = engines(E)
        for entry in ("ita_mha_long_f32", "ita_encoder_layer_long_f32"):
            for seq_len in (0, 200, 65664):
                assert _status(eng, entry, seq_len) == -4, (E, entry, seq_len)
        # the same handle still runs a valid call correctly
        want, e_torch = lc.attn_ref("plain", E, 256, 2, 0)
        _check(eng.mha_long_f32(cu(lc.inputs("plain", E, 256, 2))).cpu().numpy(), want, e_torch, f"after refusals E={E}")
        with pytest.raises(host.ITAError, match="expected"):
            eng.mha_long_f32(cu(np.zeros((1, 128, E + 4), np.float32)))


# ---- 9: camera frames
@pytest.mark.parametrize("E", [64, 128])
def test_encode_frames_long_f32_is_tokenize_then_encode(engines, E):
    import torch
    eng = engines(E)
    frames = cu(np.random.RandomState(E).randint(0, 256, (2, 97, 131)).astype(np.uint8))
    for th, tw in ((8, 16), (16, 16)):
        got = eng.encode_frames_long_f32(frames, th, tw)
        assert tuple(got.shape) == (2, th * tw, E) and bool(torch.isfinite(got).all())
        assert torch.equal(got, eng.encode_long_f32(eng.tokenize_long(frames, th, tw))), (th, tw)
