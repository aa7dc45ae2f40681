"""The float attention on rows where many keys carry weight, on the MI355X.

With the stock synthetic weights softmax(Q K^T) is almost a hard maximum (test_float_flat_cpu.py: a median of one or two
keys above 1e-4 per row), so P V is checked as a gather of one V row.  Here q_proj of the layer under test is multiplied by
s = 0, 1/64 or 1/8 (float_flat_common.py): the 128-key row sum across the four slot lanes, the reciprocal, the key order of
the context GEMM and, in the long kernel, the rescale of a running sum to which every 64-key unit contributes all decide
the result.  ita_mha_f32, ita_encoder_layer and ita_mha_long_f32 against the float64 restatement under the project's rule
(long_f32_common.bound: 3 x torch's own f32 error on the same rows, never below 1e-5); at s = 0, where every probability
is exactly 2^-7, all 128 rows of a frame are bit-equal; duplicated tokens in waves 0, 4 and 7 give bit-equal rows; a frame
holding a NaN or an inf leaves every other frame of a batch larger than the grid untouched.

Every case prints a line "flat: ..." with err, e_torch and their ratio (profiles/float_flat.txt is that output)."""
import numpy as np
import pytest

from drone_oa_iree_vit_accelerator_amd import host
from gpu_support import cu
import float_flat_common as fc
import long_f32_common as lc
from long_f32_common import LAYERS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    """engine(E, layer, s): one Engine per blob, made on first use, all closed at the end; s = 1 is the stock blob"""
    made = {}

    def get(E, layer, s):
        key = (E, 0, 1.0) if s == 1 else (E, layer, s)
        if key not in made:
            made[key] = host.Engine(fc.case(*key)[1], device=0)
            assert [made[key].attn_kind(l) for l in range(LAYERS[E])] == [host.ATTN_F32] * LAYERS[E]
        return made[key]

    yield get
    for eng in made.values():
        eng.close()


def _check(got, want, e_torch, what):
    """prints err, e_torch and their ratio, then asserts: every output finite, err within the rule's bound"""
    assert np.isfinite(got).all(), what
    err = float(np.abs(got - want).max())
    print(f"flat: {what}: |gpu - float64| = {err:.3e}, |torch f32 - float64| = {e_torch:.3e}, err / e_torch = {err / e_torch:.2f}, "
          f"bound {lc.bound(e_torch):.1e}")
    assert err <= lc.bound(e_torch), (what, err, e_torch)


FLAT = pytest.mark.parametrize("s", fc.SCALES, ids=lambda s: "s=" + fc.label(s).replace("/", "_"))
EMBED = pytest.mark.parametrize("E", [64, 128])
KIND = pytest.mark.parametrize("kind", fc.KINDS)


@FLAT
@EMBED
@KIND
def test_mha_f32_flat_rows(engine, kind, E, s):
    S, B = fc.SHORT
    x = cu(lc.inputs(kind, E, S, B))
    for l in range(LAYERS[E]):
        want, e_torch = fc.attn_ref(kind, E, S, B, l, s)
        _check(engine(E, l, s).mha_f32(x, l).cpu().numpy(), want, e_torch, f"mha_f32 s={fc.label(s)} {kind} E={E} S={S} B={B} layer {l}")


@FLAT
@EMBED
@KIND
def test_encoder_layer_flat_rows(engine, kind, E, s):
    S, B = fc.SHORT
    x = cu(lc.inputs(kind, E, S, B))
    for l in range(LAYERS[E]):
        want, e_torch = fc.layer_ref(kind, E, S, B, l, s)
        _check(engine(E, l, s).encoder_layer(x, l).cpu().numpy(), want, e_torch,
               f"encoder_layer s={fc.label(s)} {kind} E={E} S={S} B={B} layer {l}")


@pytest.mark.parametrize("S,B", fc.LONG)
@FLAT
@EMBED
@KIND
def test_mha_long_f32_flat_rows(engine, kind, E, s, S, B):
    """every 64-key unit contributes to every row's running sum; on the ramped rows the maximum keeps moving as well"""
    x = cu(lc.inputs(kind, E, S, B))
    for l in range(LAYERS[E]):
        want, e_torch = fc.attn_ref(kind, E, S, B, l, s)
        _check(engine(E, l, s).mha_long_f32(x, l).cpu().numpy(), want, e_torch,
               f"mha_long_f32 s={fc.label(s)} {kind} E={E} S={S} B={B} layer {l}")


@EMBED
@KIND
def test_scale_zero_rows_bit_equal(engine, kind, E):
    """s = 0: Q is exactly 0, every logit 0, every probability 2^-7, so each row of a frame is the same chain over the
    same V in the same key order.  A row that differs from row 0 belongs to a wave that read K or V while another wave
    was still writing it (or that walked the keys in another order)."""
    S, B = fc.SHORT
    x = cu(lc.inputs(kind, E, S, B))
    for l in range(LAYERS[E]):
        y = engine(E, l, 0.0).mha_f32(x, l).cpu().numpy()
        assert np.isfinite(y).all()
        for b in range(B):
            rows = np.flatnonzero((y[b] != y[b, :1]).any(-1))
            assert rows.size == 0, (kind, E, l, b, "rows (wave = row // 16) that differ from row 0:", rows.tolist())
        assert not np.array_equal(y[0], y[1])   # the frames themselves differ


@pytest.mark.parametrize("E", [64, 128])
def test_duplicated_tokens_stock_weights(engine, E):
    """tokens 77 and 120 are copies of token 3 (waves 4, 7 and 0): their rows of ita_mha_f32 and of the whole layer are
    bit-equal, and the output stays within the rule's bound of float64"""
    import torch
    fp, _, twin = lc.case(E)
    xn = fc.duplicated(E)
    x = cu(xn)
    eng = engine(E, 0, 1.0)
    for l in range(LAYERS[E]):
        want = lc.attn64(xn, fp, l)
        with torch.no_grad():
            e_torch = float(np.abs(twin._attention(torch.from_numpy(xn.copy()), l).numpy() - want).max())
        lwant = lc.layer64(xn, fp, l)
        le_torch = float(np.abs(lc.layer_torch(twin, xn, l) - lwant).max())
        for name, y, w, e in (("mha_f32", eng.mha_f32(x, l), want, e_torch), ("encoder_layer", eng.encoder_layer(x, l), lwant, le_torch)):
            y = y.cpu().numpy()
            assert np.array_equal(y[:, 3], y[:, 77]) and np.array_equal(y[:, 3], y[:, 120]), (name, E, l)
            assert not np.array_equal(y[:, 3], y[:, 4])
            _check(y, w, e, f"{name} duplicated tokens E={E} layer {l}")


@pytest.mark.parametrize("poison", [np.nan, np.inf], ids=["nan", "inf"])
@pytest.mark.parametrize("E", [64, 128])
def test_poisoned_frame_stays_alone(engine, E, poison):
    """a batch of CUs + 1 frames whose frame 0 holds one NaN / +inf: workgroup 0 of the attention takes frame 0 and then
    frame CUs, the FFN workgroups of tiles 0..3 go on to tiles 2 CUs.. and 4 CUs..; every frame but frame 0 equals the clean
    batch bit for bit.  Nothing is asserted about frame 0 itself."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B = cus + 1
    assert B > cus and 4 * B > 2 * (2 * cus)   # frame 0's workgroups all run at least one more iteration
    eng = engine(E, 0, 1.0)
    clean = lc.ln_like(B, 128, E, 900 + E)
    bad = clean.copy()
    bad[0, 37, 5] = poison
    xc, xb = cu(clean), cu(bad)
    for l in range(LAYERS[E]):
        for name, fn in (("mha_f32", eng.mha_f32), ("encoder_layer", eng.encoder_layer)):
            want, got = fn(xc, l).cpu().numpy(), fn(xb, l).cpu().numpy()
            assert np.isfinite(want).all()
            frames = np.flatnonzero((got[1:] != want[1:]).reshape(B - 1, -1).any(1)) + 1
            assert frames.size == 0, (name, E, l, "frames changed by the poisoned frame 0 (frame % CUs = attention workgroup):", frames.tolist()[:16])
