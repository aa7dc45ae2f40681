"""The default tail (tail mode 1: folded f16x3 GEMM, split-precision LSTM layers, v_exp_f32 / v_rcp_f32 gates) held to
float64 at its edges.  References, cases and the bound are tests/tail_f64_common.py's; tests/test_tail_f64_cpu.py shows on
the CPU that a kernel which dropped a cross term, flushed f16 subnormals, skipped a k-step or overflowed in tanh would land
outside twice that bound on these cases.

    test_within_bound            Engine.tail against truth64 under 3 (max e_f32 + max e_split) + 4 ulp32(max |truth64|) per tensor
    test_exact_mode_equals_oracle  tail mode 0 equals the f32 oracle bit for bit (W3: ita_expf's clamp at -87 / 88, both sides)
    test_kernel_independence     a frame's result does not depend on the GEMM kernel that served its batch (5 / 33 / 257 rows)
    test_forward_path_planes     x2 split in the encoder epilogue (Engine.forward) equals x2 split by ita_split_planes_kernel
    test_sequence_equals_steps_saturated  the sequence kernel's own copies of the shared blocks, on saturated gates
    test_recurrence              R1: 64 steps with a long memory, every step under that step's bound"""
import numpy as np
import pytest

import tail_f64_common as tc
from drone_oa_iree_vit_accelerator_amd import synth
from gpu_support import cu, engine_pool

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engines():
    """one engine per parameter set (loading a blob builds the fold), shared by the tests below and left in tail mode 1"""
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    yield from engine_pool(lambda key, fp: tc.blob(fp), lambda key, fp: key)


def _engine(engines, name):
    cs = tc.case(name)
    return engines("seed0" if name[0] == "A" else name, cs["fp"])


def _tail(eng, x2, dv, q, h_in, c_in):
    import torch
    vel, (h, c) = eng.tail(cu(x2), cu(dv), cu(q), (cu(h_in), cu(c_in)))
    torch.cuda.synchronize()
    assert eng.head_status() == 0
    return dict(vel=vel.cpu().numpy(), h=h.cpu().numpy(), c=c.cpu().numpy())


def _tail_case(eng, cs, rows=None):
    """Engine.tail on the case's frames, or on those frames tiled to `rows`"""
    x2, dv, q, h_in, c_in = cs["x2"], cs["desvel"], cs["quat"], cs["h_in"], cs["c_in"]
    if rows is not None:
        idx = np.arange(rows) % len(x2)
        x2, dv, q, h_in, c_in = x2[idx], dv[idx], q[idx], h_in[:, idx], c_in[:, idx]
    return _tail(eng, x2, dv, q, h_in, c_in)


def _report(what, got, truth, b, e32, esp, mask=None):
    """prints e_gpu, e_f32, e_split and e_gpu / bound per tensor; returns the tensors over their bound"""
    eg = tc.errors(got, truth, mask)
    over = []
    for n in tc.TENSORS:
        print(f"{what} {n}: e_gpu {eg[n]:.3e}  e_f32 {e32[n]:.3e}  e_split {esp[n]:.3e}  e_gpu/bound {eg[n] / b[n]:.3f}")
        if not eg[n] <= b[n]:
            over.append((n, eg[n], b[n]))
    return over


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_same_bits(got, want, what):
    for n in ("vel", "h", "c"):
        np.testing.assert_array_equal(_bits(got[n]), _bits(want[n]), err_msg=f"{what} {n}")


@pytest.mark.parametrize("name", tc.CASES)
def test_within_bound(engines, name):
    cs = tc.case(name)
    truth, _, _, b, e32, esp = tc.refs(name)
    got = _tail_case(_engine(engines, name), cs)
    assert all(np.isfinite(got[n]).all() for n in ("vel", "h", "c")), "non-finite output"
    over = _report(name, got, truth, b, e32, esp, cs["mask"])
    assert not over, over


@pytest.mark.parametrize("name", tc.CASES)
def test_exact_mode_equals_oracle(engines, name):
    cs = tc.case(name)
    eng = _engine(engines, name)
    eng.set_tail_mode(0)
    try:
        got = _tail_case(eng, cs)
    finally:
        eng.set_tail_mode(1)
    _assert_same_bits(got, tc.refs(name)[1], name)


@pytest.mark.parametrize("name", ["A1", "A4", "W1", "W3"])
def test_kernel_independence(engines, name):
    """5 rows: the tiny GEMM kernel, 33: the small one, 257: the large one (a last 128-row tile of one frame)"""
    cs = tc.case(name)
    eng = _engine(engines, name)
    ref = _tail_case(eng, cs, rows=5)
    for rows in (33, 257):
        got = _tail_case(eng, cs, rows=rows)
        _assert_same_bits({n: got[n][:5] if n == "vel" else got[n][:, :5] for n in got}, ref, f"{name} rows={rows}")
        # and the tiled copies of a frame, wherever they sit in the batch
        B = len(cs["x2"])
        for r in (rows - 1, 32):
            np.testing.assert_array_equal(_bits(got["h"][:, r]), _bits(got["h"][:, r % B]), err_msg=f"{name} rows={rows} row {r}")


@pytest.mark.parametrize("name", ["A1", "W3"])
def test_forward_path_planes(engines, name):
    """Engine.forward hands x2 to the folded GEMM as hi / lo planes written by the encoder epilogue; Engine.tail splits an
    f32 x2 in ita_split_planes_kernel.  The x2 tap of forward, fed to tail, gives forward's own vel, h and c bit for bit.
    A1: norms2.0 weight and bias times 2^-6, so the x2 the encoder emits has f16-subnormal lo halves."""
    import torch
    cs = tc.case(name)
    if name == "A1":
        fp = dict(cs["fp"])
        for k in ("norms2.0.weight", "norms2.0.bias"):
            fp[k] = fp[k] * np.float32(2.0 ** -6)
        eng = engines("A1_small_norm", fp)
    else:
        eng = _engine(engines, name)
    B = len(cs["x2"])
    fr = synth.frames(70, B)
    dv, q, hid = cu(cs["desvel"]), cu(cs["quat"]), (cu(cs["h_in"]), cu(cs["c_in"]))
    vel, (h, c), tp = eng.forward(cu(fr["img_u8"]), dv, q, hid, taps=True)
    vel2, (h2, c2) = eng.tail(tp["x2"], dv, q, hid)
    torch.cuda.synchronize()
    assert eng.head_status() == 0
    x2 = tp["x2"].cpu().numpy()
    if name == "A1":
        lo = tc.split_f16(x2)[1].astype(np.float64)
        assert np.abs(x2).max() < 0.1 and ((lo != 0) & (np.abs(lo) < tc.F16_MIN_NORMAL)).sum() > 0.9 * (lo != 0).sum()
    assert torch.isfinite(vel).all() and torch.isfinite(h).all() and torch.isfinite(c).all()
    assert torch.equal(vel.view(torch.int32), vel2.view(torch.int32)), "vel"
    assert torch.equal(h.view(torch.int32), h2.view(torch.int32)), "h"
    assert torch.equal(c.view(torch.int32), c2.view(torch.int32)), "c"


def test_sequence_equals_steps_saturated(engines):
    """W3's blob, T = 12, B = 5, lengths [12, 7, 1, 0, 12]: forward_sequence in one launch equals the step path bit for
    bit and stays finite (the sequence kernel spells the f32 -> hi, lo split, the pre-activation and the wave sums out on
    its own: the blocks marked "not shared" in ita_lstm_seq_kernel.h)"""
    import torch
    T, B, lens = 12, 5, [12, 7, 1, 0, 12]
    cs = tc.case("W3")
    eng = _engine(engines, "W3")
    eng.reserve(T * B)
    assert eng._reserved // B >= T
    fr = synth.frames(71, T * B)
    img = fr["img_u8"].reshape(T, B, 60, 90)
    dv, q = fr["desvel"].reshape(T, B), fr["quat"].reshape(T, B, 4)
    h0, c0 = cs["h_in"][:, :B], np.ascontiguousarray(cs["c_in"][:, 3:8])        # c_in of -1, +-20, +-50
    vel = torch.full((T, B, 3), -77.0, device="cuda")
    h, c = cu(h0), cu(c0)
    eng.forward_sequence(cu(img), cu(dv), cu(q), (h.clone(), c.clone()), lengths=torch.tensor(lens), out=(vel, h, c))
    torch.cuda.synchronize()
    assert eng.head_status() == 0
    vel, h, c = vel.cpu().numpy(), h.cpu().numpy(), c.cpu().numpy()
    assert np.isfinite(vel).all() and np.isfinite(h).all() and np.isfinite(c).all()
    for b, n in enumerate(lens):
        st = (cu(h0[:, b:b + 1]), cu(c0[:, b:b + 1]))
        for t in range(n):
            v, st = eng.forward(cu(img[t, b:b + 1]), cu(dv[t, b:b + 1]), cu(q[t, b:b + 1]), st)
            np.testing.assert_array_equal(_bits(vel[t, b]), _bits(v.cpu().numpy()[0]), err_msg=f"vel stream {b} step {t}")
        assert eng.head_status() == 0
        np.testing.assert_array_equal(_bits(h[:, b]), _bits(st[0].cpu().numpy()[:, 0]), err_msg=f"h stream {b}")
        np.testing.assert_array_equal(_bits(c[:, b]), _bits(st[1].cpu().numpy()[:, 0]), err_msg=f"c stream {b}")
        assert (vel[n:, b] == -77.0).all(), f"stream {b}: rows behind its length were written"


def test_recurrence(engines):
    """R1: forget-gate bias + 3, 64 steps of Engine.tail with the state carried on the device, four x2 sets cycled, B = 4;
    every step against the float64 recurrence under the bound of the f32 and the split recurrence at that step"""
    import torch
    cs, steps = tc.recurrence()
    eng = engines("R1", cs["fp"])
    x2 = [cu(cs["x2"][i]) for i in range(4)]
    side = [(cu(dv), cu(q)) for dv, q in cs["side"]]
    st = (cu(cs["h_in"]), cu(cs["c_in"]))
    outs = []
    for t in range(tc.R1_STEPS):
        vel, st = eng.tail(x2[t % 4], *side[t % 4], st)
        outs.append((vel, st[0], st[1]))
    torch.cuda.synchronize()
    assert eng.head_status() == 0
    over, worst = [], {n: (0.0, 0, 0.0, 0.0, 0.0) for n in tc.TENSORS}
    for t, ((vel, h, c), (truth, b, e32, esp)) in enumerate(zip(outs, steps)):
        eg = tc.errors(dict(vel=vel.cpu().numpy(), h=h.cpu().numpy(), c=c.cpu().numpy()), truth)
        for n in tc.TENSORS:
            if eg[n] / b[n] >= worst[n][0]:
                worst[n] = (eg[n] / b[n], t, eg[n], e32[n], esp[n])
            if not eg[n] <= b[n]:
                over.append((t, n, eg[n], b[n]))
    for n in tc.TENSORS:
        r, t, eg, e3, es = worst[n]
        print(f"R1 {n}: worst step {t}: e_gpu {eg:.3e}  e_f32 {e3:.3e}  e_split {es:.3e}  e_gpu/bound {r:.3f}")
    assert not over, over[:8]
