"""Shared by the long float taps tests (test_long_f32_taps_cpu.py, test_gpu_long_f32_taps.py): per-tensor references for
ita_mha_long_f32_taps -- q, k, v, q k^T, softmax, p v of ITASelfAttention.forward in float64 and in torch's CPU f32 --
the bounds they set, the query rows the tests choose, and an f32 numpy emulation of the flash sweep of
csrc/ita_long_f32_kernel.h (block-summed projections and logits, 64-key units, running m and l, the four lane shares
added at the end, ita_expf through oracle.lib().ita_oracle_expf).  Everything cached here is read-only.

Bounds (the project's rule; e_torch is torch's own error against float64 on the same rows, never GPU output):
  Q, K, V, logits, ctx   3 e_torch + 4 ulp32(max |truth64|) per case and tensor
  probs                  long_f32_common.bound(e_torch)
  row_sum, relative      max(1e-5, 3 e_torch_rel); torch's row sum is sum(exp(s - max s)) of its own f32 logits"""
import functools

import numpy as np

import long_f32_common as lc

TENSORS = ("Q", "K", "V", "ctx")


def ulp32(v):
    return float(np.spacing(np.float32(abs(v))))


def expf(a):
    """ita_expf (the oracle's scalar, element by element) over an f32 array"""
    from oracle import oracle
    f = oracle.lib().ita_oracle_expf
    a = np.ascontiguousarray(a, np.float32)
    return np.fromiter((f(float(v)) for v in a.ravel()), np.float32, a.size).reshape(a.shape)


def _w(fp, layer, dt):
    g = lambda k: fp[f"attention_blocks.{layer}.{k}"].astype(dt)
    return {n: (g(f"{n}_proj.weight"), g(f"{n}_proj.bias")) for n in "qkv"}


@functools.lru_cache(maxsize=None)
def refs(kind, E, S, B, layer=0):
    """(truth64, torch32): dicts of Q, K, V (B,S,P), logits, probs (B,S,S), ctx (B,S,P), row_sum (B,S) -- float64
    restatement, and torch's f32 evaluation of the same tensors on the CPU"""
    import torch
    fp, _, _ = lc.case(E)
    x = lc.inputs(kind, E, S, B)
    w = _w(fp, layer, np.float64)
    x64 = x.astype(np.float64)
    t = {n.upper(): x64 @ w[n][0].T + w[n][1] for n in "qkv"}
    t["logits"] = t["Q"] @ t["K"].transpose(0, 2, 1)
    e = np.exp(t["logits"] - t["logits"].max(-1, keepdims=True))
    t["row_sum"] = e.sum(-1)
    t["probs"] = e / t["row_sum"][..., None]
    t["ctx"] = t["probs"] @ t["V"]
    with torch.no_grad():
        F = torch.nn.functional
        xt = torch.from_numpy(x.copy())
        w32 = {n: (torch.from_numpy(a.astype(np.float32)), torch.from_numpy(b.astype(np.float32))) for n, (a, b) in _w(fp, layer, np.float32).items()}
        r = {n.upper(): F.linear(xt, *w32[n]) for n in "qkv"}
        r["logits"] = torch.matmul(r["Q"], r["K"].transpose(-2, -1))
        r["row_sum"] = torch.exp(r["logits"] - r["logits"].max(-1, keepdim=True).values).sum(-1)
        r["probs"] = torch.softmax(r["logits"], dim=-1)
        r["ctx"] = torch.matmul(r["probs"], r["V"])
        r = {k: v.numpy() for k, v in r.items()}
    for d in (t, r):
        for v in d.values():
            v.setflags(write=False)
    return t, r


@functools.lru_cache(maxsize=None)
def rows_for(kind, E, S, B, layer=0):
    """the boundary rows {0, 15, 16, 127, 128, S - 129, S - 1} in [0, S), plus the four rows of frame 0 whose largest
    float64 probability is smallest: a one-hot row (56-76 % of the rows with these weights) does not test row_sum"""
    t, _ = refs(kind, E, S, B, layer)
    top = t["probs"][0].max(-1)
    soft = [int(i) for i in np.argsort(top, kind="stable")[:4]]
    assert all(top[i] < 0.9 for i in soft), (kind, E, S, B, layer, top[soft])
    return tuple(sorted({r for r in (0, 15, 16, 127, 128, S - 129, S - 1) if 0 <= r < S} | set(soft)))


def bounds(kind, E, S, B, layer, rows):
    """tap -> (bound, e_torch) on this case; logits, probs and row_sum (relative) on the chosen rows"""
    t, r = refs(kind, E, S, B, layer)
    rows = list(rows)
    out = {}
    for k in TENSORS + ("logits",):
        a, b = (t[k][:, rows], r[k][:, rows]) if k == "logits" else (t[k], r[k])
        e = float(np.abs(b - a).max())
        out[k] = (3.0 * e + 4.0 * ulp32(np.abs(a).max()), e)
    e = float(np.abs(r["probs"][:, rows] - t["probs"][:, rows]).max())
    out["probs"] = (lc.bound(e), e)
    e = float((np.abs(r["row_sum"][:, rows] - t["row_sum"][:, rows]) / t["row_sum"][:, rows]).max())
    out["row_sum"] = (max(1e-5, 3.0 * e), e)
    return out


def errors(got, kind, E, S, B, layer, rows):
    """tap -> error of `got` (a dict of taps as the entry returns them) against float64, in the unit of its bound"""
    t, _ = refs(kind, E, S, B, layer)
    rows = list(rows)
    out = {}
    for k in got:
        g = np.asarray(got[k], np.float64)
        if k in TENSORS:
            out[k] = float(np.abs(g - t[k]).max())
        elif k in ("logits", "probs"):
            out[k] = float(np.abs(g - t[k][:, rows]).max())
        elif k == "row_sum":
            out[k] = float((np.abs(g - t[k][:, rows]) / t[k][:, rows]).max())
    return out


# ---- the f32 emulation of the two launches
def _fma(a, b, c):
    """fmaf: the f32 product is exact in float64, one rounding of the sum to f32 follows"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _order16():
    """the k order of four 16x16x4 MFMAs over a 16-wide group: MFMA r chains slots 0..3, element 4 slot + r"""
    return [4 * s + r for r in range(4) for s in range(4)]


def _project(x, w, b, block):
    """x (B,S,E) f32, w (P,E), b (P): block sums (16 products chained from zero, then added to the total seeded with the
    bias) or, block=False, one fmaf chain from the bias"""
    acc = np.broadcast_to(b.astype(np.float32), x.shape[:2] + (w.shape[0],)).copy()
    for g in range(x.shape[2] // 16):
        t = np.zeros_like(acc) if block else acc
        for j in _order16():
            t = _fma(x[:, :, 16 * g + j, None], w[None, None, :, 16 * g + j], t)
        acc = (acc + t).astype(np.float32) if block else t
    return acc


def _logits(q, k, block):
    """q, k (B,S,P) f32 -> (B,S,S): twelve 16-feature blocks chained from zero and added in order, or one chain"""
    s = np.zeros((q.shape[0], q.shape[1], k.shape[1]), np.float32)
    for ft in range(q.shape[2] // 16):
        t = np.zeros_like(s) if block else s
        for j in _order16():
            t = _fma(q[:, :, None, 16 * ft + j], k[:, None, :, 16 * ft + j], t)
        s = (s + t).astype(np.float32) if block else t
    return s


def emulate(kind, E, S, B, layer, rows, mutation=None):
    """the taps of ita_mha_long_f32_taps as the kernels' arithmetic gives them, in numpy f32.  mutation: one of the wrong
    kernels test_long_f32_taps_cpu.py must tell from the right one:
      'max_at_unit'   probs from the running maximum of the unit a key sits in, not the final one
      'lane_missing'  row_sum without the fourth lane share
      'no_rescale'    row_sum without the e^(m - m') factor
      'unit_swapped'  the logits of unit u stored at unit u ^ 1
      'one_lane_sum'  probs divided by one lane's share of the sum
      'one_chain'     Q, K and the logits as one fmaf chain from the bias, K's feature tiles 0 and 1 swapped"""
    fp, _, _ = lc.case(E)
    x = lc.inputs(kind, E, S, B)
    w = _w(fp, layer, np.float32)
    block = mutation != "one_chain"
    Q, K = _project(x, *w["q"], block), _project(x, *w["k"], block)
    V = _project(x, *w["v"], True)
    if mutation == "one_chain":
        K = np.concatenate([K[..., 16:32], K[..., :16], K[..., 32:]], -1)
    s = _logits(Q, K, block)
    m = np.full((B, S), -np.inf, np.float32)
    l = np.zeros((B, S, 4), np.float32)             # the four lane shares: slot holds keys 16 kt + 4 slot + r of a unit
    c = np.zeros((B, S, 192), np.float32)
    m_at = np.empty((B, S, S // 64), np.float32)
    for u in range(S // 64):
        su = s[:, :, 64 * u:64 * u + 64]
        mn = np.maximum(m, su.max(-1))
        down = expf(m - mn)                         # first unit: -inf, the clamp's e^-87, times l = 0 and c = 0
        m = mn
        m_at[:, :, u] = m
        e = expf(su - mn[..., None])
        share = np.zeros((B, S, 4), np.float32)
        for kt in range(4):
            for r in range(4):
                share = (share + e[:, :, 16 * kt + r:16 * kt + 16:4]).astype(np.float32)
        l = share + l if mutation == "no_rescale" else (l * down[..., None]).astype(np.float32) + share
        l = l.astype(np.float32)
        c = (c * down[..., None]).astype(np.float32)
        for kt in range(4):
            for r in range(4):
                for slot in range(4):
                    key = 16 * kt + 4 * slot + r
                    c = _fma(V[:, None, 64 * u + key, :], e[:, :, key, None], c)
    a, b = (l[..., 0] + l[..., 1]).astype(np.float32), (l[..., 2] + l[..., 3]).astype(np.float32)
    row_sum = (a + (l[..., 2] if mutation == "lane_missing" else b)).astype(np.float32)
    ctx = (c * (np.float32(1.0) / row_sum)[..., None]).astype(np.float32)
    rows = list(rows)
    lg, mx, sm = s[:, rows], m[:, rows], row_sum[:, rows]
    if mutation == "unit_swapped":
        lg = lg.reshape(B, len(rows), S // 64, 64)[:, :, np.arange(S // 64) ^ 1].reshape(B, len(rows), S)
    sub = mx[..., None]
    if mutation == "max_at_unit":
        sub = np.repeat(m_at[:, rows], 64, axis=-1)
    div = l[:, rows, 0] if mutation == "one_lane_sum" else sm
    probs = (expf(lg - sub) * (np.float32(1.0) / div)[..., None]).astype(np.float32)
    return dict(Q=Q, K=K, V=V, ctx=ctx, logits=lg, probs=probs, row_max=mx, row_sum=sm)
