"""Shared by the default-tail tests (test_tail_f64_cpu.py, test_gpu_tail_f64.py): references of the graph behind the encoder,
from x2 (B,128,64), desvel, quat and the state (h_in, c_in) on, for the E = 64 tail family.  Everything here runs on the CPU.

    truth64   float64 throughout: FloatTwin.forward restated from x2 on (pixel_shuffle || bilinear upsample -> conv3x3 ->
              decoder -> cat -> three LSTM cells -> fc)
    oracle32  the f32 oracle's composition oracle.tail -> oracle.linear_f32 -> oracle.head_from_dec
    split64   tail mode 1's DESIGN with exact sums: G0 = W_ih0[:, :512] . Wdec . T built in float64 and rounded to f32,
              weights scaled by the power of two of split_scale_exp and split like split_half, activations split like
              split_f16, lo_x.hi_w + hi_x.lo_w + hi_x.hi_w accumulated in float64; biases, gates, cell update, fc in float64
    mutants   of split64, for the CPU sensitivity assertions: what a subtly wrong kernel would compute

e_f32 = |oracle32 - truth64| is what f32 arithmetic costs on a case, e_split = |split64 - truth64| what the design accepts.
A GPU result is held to   3 (max e_f32 + max e_split) + 4 ulp32(max |truth64|)   per case and output tensor: no absolute
floor, nothing taken from GPU output.  Cached results are read-only."""
import functools
import hashlib

import numpy as np

from conftest import golden_files
from drone_oa_iree_vit_accelerator_amd import params, synth

TENSORS = ("vel", "h0", "h1", "h2", "c0", "c1", "c2")
MUTANTS = ("no_x_lo", "no_w_lo", "flush_f16_subnormals", "tanh_ratio")   # and ("skip_k_step", k0)
IMPULSE_K = (0, 7, 8, 31, 32, 63, 64, 1023, 1024, 8191)   # fragment, k-step, k-tile and K-slice seams of the folded GEMM (NSPLIT = 8)
SAT_TARGETS = (0.0, 1e-6, -1e-6, 20.0, -20.0, 50.0, -50.0, 90.0, -90.0, 130.0, -130.0, 200.0, -200.0)
F16_MIN_NORMAL = 2.0 ** -14


def _f64(a):
    return np.asarray(a, np.float64)


def _key(*arrays):
    h = hashlib.sha1()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


@functools.lru_cache(maxsize=None)
def record():
    return params.load_fixture(golden_files("vitlstm_E64_seed0_B2.npz")[0])


@functools.lru_cache(maxsize=None)
def seed0_params():
    fp = synth.float_params(0, E=64)
    for v in fp.values():
        v.setflags(write=False)
    return fp


# ------------------------------------------------------------------ split-precision arithmetic (ita_weights_load.h, ita_f16x3_kernels.h)
def split_scale_exp(max_abs):
    """max|w| . 2^e in [512, 1024)"""
    if not max_abs > 0.0:
        return 0
    return 10 - int(np.frexp(np.float32(max_abs))[1])


def split_f16(x):
    """hi = half(x), lo = half(x - hi) of f32 values (round to nearest even, f16 subnormals kept): split_f16 on the device,
    split_half on the host"""
    x = np.asarray(x, np.float32)
    with np.errstate(over="ignore"):
        hi = x.astype(np.float16)
        lo = (x - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def split_weights(w):
    """split_upload: one scale for the tensor, then split_half -> (hi, lo as f16 arrays of w . 2^e, e)"""
    w = np.asarray(w, np.float32)
    e = split_scale_exp(float(np.abs(w).max()))
    hi, lo = split_f16(w * np.float32(2.0 ** e))
    return hi, lo, e


def flush_f16(a):
    a = np.array(a, np.float64)
    a[np.abs(a) < F16_MIN_NORMAL] = 0.0
    return a


def split_dot(x, wsplit, mutant=None, skip_k0=None):
    """x (B,K) f32 activations, unscaled; wsplit = split_weights of (N,K): x . w^T with the three products summed in float64"""
    wh, wl, e = wsplit
    xh, xl = (_f64(a) for a in split_f16(x))
    wh, wl = _f64(wh), _f64(wl)
    if mutant == "flush_f16_subnormals":
        xh, xl, wh, wl = flush_f16(xh), flush_f16(xl), flush_f16(wh), flush_f16(wl)
    if skip_k0 is not None:
        xh, xl = xh.copy(), xl.copy()
        xh[:, skip_k0:skip_k0 + 32] = 0.0
        xl[:, skip_k0:skip_k0 + 32] = 0.0
    acc = xh @ wh.T
    if mutant != "no_x_lo":
        acc = acc + xl @ wh.T
    if mutant != "no_w_lo":
        acc = acc + xh @ wl.T
    return acc * 2.0 ** -e


# ------------------------------------------------------------------ the fusion tail and the fold in float64
def _upsample_matrix(n_in, n_out):
    """bilinear, align_corners=True: (n_out, n_in)"""
    U = np.zeros((n_out, n_in))
    for d in range(n_out):
        src = d * (n_in - 1) / (n_out - 1)
        i0 = min(int(np.floor(src)), n_in - 1)
        U[d, i0] += 1.0 - (src - i0)
        if i0 < n_in - 1:
            U[d, i0 + 1] += src - i0
    return U


def feat64(x2, fp):
    """x2 (B,128,E) -> the decoder's input (B,4608), torch in double (the ops FloatTwin.forward uses)"""
    import torch
    F = torch.nn.functional
    x = torch.from_numpy(_f64(x2))
    B, _, E = x.shape
    x2d = x.transpose(1, 2).reshape(B, E, 8, 16)
    fused = torch.cat([F.pixel_shuffle(x2d, 2), F.interpolate(x2d, size=(16, 32), mode="bilinear", align_corners=True)], 1)
    cw, cb = (torch.from_numpy(_f64(fp[k])) for k in ("down_sample.weight", "down_sample.bias"))
    return F.conv2d(fused, cw, cb, padding=1).flatten(1).numpy()


_WFOLD = {}


def wfold64(fp):
    """(Wfold (512, 8192) = Wdec . T with T the bias-free fusion tail, bias' (512) = dec(tail(0))) in float64.  Built
    directly, by the transposed maps: every decoder row goes back through the conv3x3 (conv_transpose2d), the pixel shuffle
    (pixel_unshuffle) and the upsampling (U^T . V); feat64 is the forward statement it is tested against."""
    import torch
    F = torch.nn.functional
    k = _key(fp["down_sample.weight"], fp["down_sample.bias"], fp["decoder.weight"], fp["decoder.bias"])
    if k not in _WFOLD:
        E = fp["down_sample.weight"].shape[1] * 4 // 5
        wd = torch.from_numpy(_f64(fp["decoder.weight"])).reshape(512, 9, 16, 32)
        g = F.conv_transpose2d(wd, torch.from_numpy(_f64(fp["down_sample.weight"])), padding=1)    # (512, 5E/4, 16, 32)
        U, V = torch.from_numpy(_upsample_matrix(8, 16)), torch.from_numpy(_upsample_matrix(16, 32))
        gx = F.pixel_unshuffle(g[:, :E // 4], 2) + torch.einsum("yi,ncyx,xj->ncij", U, g[:, E // 4:], V)   # (512, E, 8, 16)
        wf = gx.permute(0, 2, 3, 1).reshape(512, 128 * E).numpy().copy()                          # k = token * E + channel
        fb = np.repeat(_f64(fp["down_sample.bias"]), 512)                                        # tail(0): the conv bias everywhere
        bias = _f64(fp["decoder.weight"]) @ fb + _f64(fp["decoder.bias"])
        wf.setflags(write=False)
        if len(_WFOLD) >= 3:
            _WFOLD.clear()
        _WFOLD[k] = (wf, bias)
    return _WFOLD[k]


_G0 = {}


def g0_split(fp):
    """(split_weights of f32(G0), bias'' of layer 0 in float64), G0 = W_ih0[:, :512] . Wfold in float64"""
    k = _key(fp["down_sample.weight"], fp["decoder.weight"], fp["decoder.bias"], fp["lstm.weight_ih_l0"])
    if k not in _G0:
        wf, bias = wfold64(fp)
        w0 = _f64(fp["lstm.weight_ih_l0"])[:, :512]
        g0 = (w0 @ wf).astype(np.float32)
        if len(_G0) >= 4:
            _G0.clear()
        _G0[k] = (g0, split_weights(g0), w0 @ bias)
    return _G0[k]


def rem0_weights(fp):
    """layer 0's remainder [W_hh0 | W_ih0[:, 512:517]] (512, 133): what the folded GEMM does not cover"""
    return np.concatenate([fp["lstm.weight_hh_l0"], fp["lstm.weight_ih_l0"][:, 512:517]], 1).astype(np.float32)


def cat_weights(fp, l):
    return np.concatenate([fp[f"lstm.weight_ih_l{l}"], fp[f"lstm.weight_hh_l{l}"]], 1).astype(np.float32)


# ------------------------------------------------------------------ gates and cell in float64
def _sigmoid(v):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-v))


def tanh_ratio_f32(v):
    """the mutant's tanh: (e^2x - 1) / (e^2x + 1) in float32 -- inf / inf past x = 44.4"""
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(np.float32(2.0) * np.asarray(v, np.float32))
        return _f64((e - np.float32(1.0)) / (e + np.float32(1.0)))


def cell64(pre, c_in, tanh=np.tanh):
    i, f, g, o = np.split(pre, 4, axis=1)
    c = _sigmoid(f) * c_in + _sigmoid(i) * tanh(g)
    return _sigmoid(o) * tanh(c), c


def _bias(fp, l):
    return _f64(fp[f"lstm.bias_ih_l{l}"]) + _f64(fp[f"lstm.bias_hh_l{l}"])


def _fc(fp, h):
    return h @ _f64(fp["nn_fc2.weight"]).T + _f64(fp["nn_fc2.bias"])


def _result(h, c, pre, vel):
    out = dict(vel=vel, h=np.stack(h), c=np.stack(c), pre=np.stack(pre))
    return out


# ------------------------------------------------------------------ the three references, front (state-free) and head
def front_truth(fp, x2):
    """decoder output in float64 (B,512)"""
    return feat64(x2, fp) @ _f64(fp["decoder.weight"]).T + _f64(fp["decoder.bias"])


def head_truth(fp, dec, desvel, quat, h_in, c_in, upto=3):
    B = dec.shape[0]
    x = np.concatenate([dec, _f64(desvel).reshape(B, 1) / 10.0, _f64(quat).reshape(B, 4)], 1)
    h, c, pre = [], [], []
    for l in range(upto):
        p = x @ _f64(fp[f"lstm.weight_ih_l{l}"]).T + _f64(h_in[l]) @ _f64(fp[f"lstm.weight_hh_l{l}"]).T + _bias(fp, l)
        hl, cl = cell64(p, _f64(c_in[l]))
        h.append(hl); c.append(cl); pre.append(p)
        x = hl
    return _result(h, c, pre, _fc(fp, x) if upto == 3 else None)


def front_oracle(fp, x2):
    from oracle import oracle
    feat = oracle.tail(np.asarray(x2, np.float32), fp["down_sample.weight"], fp["down_sample.bias"])
    return oracle.linear_f32(feat, fp["decoder.weight"], fp["decoder.bias"])


def head_oracle(fp, dec, desvel, quat, h_in, c_in):
    from oracle import oracle
    vel, h, c = oracle.head_from_dec(dec, desvel, quat, fp, np.asarray(h_in, np.float32), np.asarray(c_in, np.float32))
    return dict(vel=vel, h=h, c=c)


def front_split(fp, x2, mutant=None, skip_k0=None):
    """layer 0's pre-activation share of the folded GEMM, x2 . G0^T (B,512), bias'' included"""
    _, gs, b0 = g0_split(fp)
    x = np.asarray(x2, np.float32).reshape(len(x2), -1)
    return split_dot(x, gs, mutant, skip_k0) + b0


def head_split(fp, p0, desvel, quat, h_in, c_in, mutant=None):
    B = p0.shape[0]
    tanh = tanh_ratio_f32 if mutant == "tanh_ratio" else np.tanh
    f32 = lambda a: np.asarray(a, np.float32)
    dv = f32(desvel).reshape(B, 1) / np.float32(10.0)
    x = np.concatenate([f32(h_in[0]), dv, f32(quat).reshape(B, 4)], 1)
    pre0 = p0 + split_dot(x, split_weights(rem0_weights(fp)), mutant) + _bias(fp, 0)
    h, c, pre = [], [], []
    for l in range(3):
        if l == 0:
            p = pre0
        else:   # the device holds h as f32 and splits that
            p = split_dot(np.concatenate([f32(h[l - 1]), f32(h_in[l])], 1), split_weights(cat_weights(fp, l)), mutant) + _bias(fp, l)
        hl, cl = cell64(p, _f64(c_in[l]), tanh)
        h.append(hl); c.append(cl); pre.append(p)
    return _result(h, c, pre, _fc(fp, h[2]))


def truth64(case):
    return head_truth(case["fp"], front_truth(case["fp"], case["x2"]), case["desvel"], case["quat"], case["h_in"], case["c_in"])


def oracle32(case):
    return head_oracle(case["fp"], front_oracle(case["fp"], case["x2"]), case["desvel"], case["quat"], case["h_in"], case["c_in"])


def split64(case, mutant=None):
    skip = mutant[1] if isinstance(mutant, tuple) else None
    mutant = None if isinstance(mutant, tuple) else mutant
    fp = case["fp"]
    return head_split(fp, front_split(fp, case["x2"], mutant, skip), case["desvel"], case["quat"], case["h_in"], case["c_in"], mutant)


# ------------------------------------------------------------------ errors and the bound
def tensors(res):
    """a result's seven output tensors under the names of TENSORS"""
    out = {"vel": np.asarray(res["vel"])}
    for l in range(3):
        out[f"h{l}"], out[f"c{l}"] = np.asarray(res["h"][l]), np.asarray(res["c"][l])
    return out


def ulp32(v):
    return float(np.spacing(np.float32(abs(v))))


def _sel(a, name, mask):
    """the judged elements of tensor `name`: mask[l] (128 bool) picks the units of h[l] / c[l]; vel is always whole"""
    if mask is None or name == "vel":
        return a
    return a[..., mask[int(name[1])]]


def errors(res, truth, mask=None):
    """max |res - truth| per tensor over the judged elements; inf where res is not finite"""
    t, r = tensors(truth), tensors(res)
    out = {}
    for n in TENSORS:
        d = np.abs(_f64(_sel(r[n], n, mask)) - _sel(t[n], n, mask))
        out[n] = float("inf") if not np.isfinite(d).all() else float(d.max())
    return out


def bounds(truth, o32, s64, mask=None):
    """per tensor: 3 (max e_f32 + max e_split) + 4 ulp32(max |truth64|), and the two error terms"""
    e32, esp = errors(o32, truth, mask), errors(s64, truth, mask)
    t = tensors(truth)
    b = {n: 3.0 * (e32[n] + esp[n]) + 4.0 * ulp32(np.abs(_sel(t[n], n, mask)).max()) for n in TENSORS}
    return b, e32, esp


# ------------------------------------------------------------------ cases
CASES = ("A0", "A1", "A2", "A3", "A4", "W1", "W2", "W3", "W4_i", "W4_f", "W4_g", "W4_o")
W1_ROWS = (2 * 128 + 37, 0 * 128 + 5, 3 * 128 + 90)   # layer l's row scaled by 2^10: gate g unit 37, gate i unit 5, gate o unit 90


def _states(rs, B, scale=0.3):
    h = (scale * rs.standard_normal((3, B, 128))).astype(np.float32)
    c = (scale * rs.standard_normal((3, B, 128))).astype(np.float32)
    return h, c


def _side(rs, B):
    dv = rs.uniform(2.0, 8.0, size=(B,)).astype(np.float32)
    q = rs.standard_normal((B, 4))
    return dv, (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)


def x2_fixture(B=8):
    """the fixture's s0.x2 (two frames of the reference's own forward) tiled to B frames"""
    x = record()["s0.x2"]
    return np.ascontiguousarray(np.tile(x, ((B + 1) // 2, 1, 1))[:B])


def ln_ceiling(fp):
    """what LayerNorm norms2.0 can emit at most: one feature carrying the whole variance, sqrt(E - 1) max|w| + max|b|"""
    w, b = fp["norms2.0.weight"], fp["norms2.0.bias"]
    return float(np.sqrt(len(w) - 1.0) * np.abs(w).max() + np.abs(b).max())


def _lstm_edit(fp, fn):
    fp = dict(fp)
    for l in range(3):
        for nm in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
            k = f"lstm.{nm}_l{l}"
            fp[k] = np.ascontiguousarray(fn(nm, l, fp[k].copy()), np.float32)
    return fp


def _w3_params(fp, x2, dv, q, h_in, c_in):
    """bias_ih per unit so that frame 0's pre-activation of gate G, unit u of every layer is SAT_TARGETS[(a_G u + G) % 13]
    (a = 1, 2, 3, 5) in float64; layer by layer, since layer l's input is layer l - 1's output"""
    fp = _lstm_edit(fp, lambda nm, l, a: a)
    dec = front_truth(fp, x2)
    tgt = np.array(SAT_TARGETS)
    u = np.arange(128)
    want = np.concatenate([tgt[(a * u + g) % 13] for g, a in enumerate((1, 2, 3, 5))])
    for l in range(3):
        fp[f"lstm.bias_ih_l{l}"] = np.zeros(512, np.float32)
        pre = head_truth(fp, dec, dv, q, h_in, c_in, upto=l + 1)["pre"][l][0]
        fp[f"lstm.bias_ih_l{l}"] = (want - pre).astype(np.float32)
    return fp


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(name, fp, x2 (B,128,64), desvel (B), quat (B,4), h_in, c_in (3,B,128), mask: judged units per layer or None)"""
    fp = dict(seed0_params())
    rs = np.random.RandomState(1000 + CASES.index(name))
    B = 10 if name == "A4" else 8
    x2 = x2_fixture(B)
    dv, q = _side(rs, B)
    h_in, c_in = _states(rs, B)
    mask = None
    if name == "A1" or name == "A2":
        s = np.float32(2.0 ** (-6 if name == "A1" else -12))
        x2, h_in, q = x2 * s, h_in * s, q * s
    elif name == "A3":
        x2 = x2 * np.float32(16.0)
        top = np.float32(16.0 * ln_ceiling(fp))
        for i, (b, tok, ch) in enumerate(((6, 0, 0), (6, 64, 63), (7, 127, 31), (7, 17, 32))):
            x2[b, tok, ch] = top if i % 2 == 0 else -top
    elif name == "A4":
        x2 = np.zeros_like(x2)
        for b, k in enumerate(IMPULSE_K):
            x2.reshape(B, -1)[b, k] = np.float32(1.0 + 2.0 ** -12)
        h_in, c_in = np.zeros_like(h_in), np.zeros_like(c_in)
    elif name == "W1":
        def scale_row(nm, l, a):
            if nm.startswith("weight"):
                a[W1_ROWS[l]] *= np.float32(1024.0)
            return a
        fp = _lstm_edit(fp, scale_row)
        mask = np.ones((3, 128), bool)
        for l in range(3):
            mask[l, W1_ROWS[l] % 128] = False
    elif name == "W2":
        fp = _lstm_edit(fp, lambda nm, l, a: a * np.float32(2.0 ** -8) if nm.startswith("weight") else a)
        fp["decoder.weight"] = fp["decoder.weight"] * np.float32(64.0)
        fp["decoder.bias"] = fp["decoder.bias"] * np.float32(64.0)
    elif name == "W3":
        x2 = np.ascontiguousarray(np.tile(x2[:1], (B, 1, 1)))                  # one frame eight times: only c_in differs
        dv, q = np.tile(dv[:1], B), np.tile(q[:1], (B, 1))
        pat = np.array([1.0, -1.0, -0.0, 0.0], np.float32)[rs.randint(0, 4, size=(3, 1, 128))]
        small = (1e-3 * rs.standard_normal((3, 1, 128))).astype(np.float32)
        h_in = np.ascontiguousarray(np.tile(np.where((pat == 0) & ~np.signbit(pat), small, pat), (1, B, 1)))
        cv = np.array([0.0, -0.0, 1.0, -1.0, 20.0, -20.0, 50.0, -50.0], np.float32)
        c_in = np.ascontiguousarray(np.broadcast_to(cv[None, :, None], (3, B, 128)))
        fp = _w3_params(fp, x2, dv, q, h_in, c_in)
    elif name.startswith("W4"):
        shift = 2 - "ifgo".index(name[-1])                                       # this gate's row group moves into the g slot
        def rotate(nm, l, a):
            a = np.roll(a.reshape(4, 128, -1), shift, axis=0).reshape(a.shape)
            if nm == "bias_ih":
                a[0:128] += np.float32(30.0)
                a[384:512] += np.float32(30.0)
            return a
        fp = _lstm_edit(fp, rotate)
        c_in = np.zeros_like(c_in)
    elif name != "A0":
        raise KeyError(name)
    out = dict(name=name, fp=fp, x2=np.ascontiguousarray(x2, np.float32), desvel=dv, quat=q, h_in=h_in, c_in=c_in, mask=mask)
    for v in list(out.values()) + list(fp.values()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def refs(name):
    """(truth64, oracle32, split64, bound per tensor, e_f32 per tensor, e_split per tensor) of a case"""
    cs = case(name)
    t, o, s = truth64(cs), oracle32(cs), split64(cs)
    b, e32, esp = bounds(t, o, s, cs["mask"])
    return t, o, s, b, e32, esp


def blob(fp):
    return params.blob_from_record(record(), fp, E=64)


# ------------------------------------------------------------------ R1: the recurrence
R1_STEPS, R1_B = 64, 4


@functools.lru_cache(maxsize=None)
def recurrence():
    """forget-gate bias + 3 (long memory), 64 steps, B = 4, cycling four sets of LayerNorm-like x2 frames, state carried by
    each reference itself.  Returns (case of step inputs, per-step list of (truth64, bound, e_f32, e_split))."""
    def forget(nm, l, a):
        if nm == "bias_ih":
            a[128:256] += np.float32(3.0)
        return a
    fp = _lstm_edit(dict(seed0_params()), forget)
    rs = np.random.RandomState(2000)
    x = rs.standard_normal((4, R1_B, 128, 64))
    x = (x - x.mean(-1, keepdims=True)) / x.std(-1, keepdims=True)
    x2 = (x * fp["norms2.0.weight"] + fp["norms2.0.bias"]).astype(np.float32)
    side = [_side(rs, R1_B) for _ in range(4)]
    h0, c0 = _states(rs, R1_B)
    fr_t = [front_truth(fp, x2[i]) for i in range(4)]
    fr_o = [front_oracle(fp, x2[i]) for i in range(4)]
    fr_s = [front_split(fp, x2[i]) for i in range(4)]
    st_t = st_o = st_s = (h0, c0)
    steps = []
    for t in range(R1_STEPS):
        i = t % 4
        dv, q = side[i]
        rt = head_truth(fp, fr_t[i], dv, q, *st_t)
        ro = head_oracle(fp, fr_o[i], dv, q, *st_o)
        rsp = head_split(fp, fr_s[i], dv, q, *st_s)
        st_t, st_o, st_s = (rt["h"], rt["c"]), (ro["h"], ro["c"]), (rsp["h"], rsp["c"])
        steps.append((rt,) + bounds(rt, ro, rsp))
    return dict(fp=fp, x2=x2, side=side, h_in=h0, c_in=c0), steps
