"""Shared by the long-attention tests at S = 8192 and S = 65536 (test_long_limits_cpu.py, test_gpu_long_limits.py):
the query rows they sample, references that form K and V for all S tokens but Q, the logits and everything behind them
for the sampled rows only (a (B, S, S) float64 tensor is 32 GiB at S = 65536), wrong kernels restated in float64, an f32
model that adds every key in one chain, and the vocabulary frames of the statistics tests.  CPU only.

Nothing is restated: the inputs, the blobs and the bound are long_f32_common's, the flattened blobs float_flat_common's,
the per-tensor bounds the rules of long_f32_taps_common and long_f32_stats_common (3 e_torch + 4 ulp32(max |truth|);
probabilities lc.bound; row sums max(1e-5, 3 e_torch) relative) applied to the sampled rows, the int8 rows
long_taps_common.mha_rows.  test_long_limits_cpu.py holds every row-sampled form equal to the whole-matrix one at small S.
Everything cached here is read-only.

Vocabulary frames.  A frame of S tokens is drawn from V distinct tokens: `singles` of them stand at one position each, the
others share the remaining positions, all at seeded random positions.  Two rows with the same token have the same query
and sweep the same keys in the same order, so every row statistic is bit-equal inside a class, and
    col_mass[j] = sum_c count_c p[c, j],    col_nnz[j] = sum_c count_c [p[c, j] counts]
with one representative row per class: V rows of S keys stand for the S x S matrix, exactly."""
import functools

import numpy as np

import float_flat_common as fc
import long_f32_common as lc
import long_f32_taps_common as ltc

SIZES = ((8192, 2), (65536, 1))                 # (S, B)
MODELS = ((64, 0), (128, 0), (128, 1))          # (E, layer)
KINDS = ("plain", "ramp", "ramp_rev", "spike_last")
UNIT = 64                                       # keys per unit of the float sweep
N_RANDOM = 55
CHAIN_STEP = 8                                  # the one-chain model runs on every eighth sampled row


@functools.lru_cache(maxsize=None)
def rows_for(S, n_random=N_RANDOM):
    """rows 0, 1, 127, 128 (first query tile and its seam), S/2 - 1, S/2, S - 129, S - 128, S - 1 (the last tile, the last
    entry of the row table) and n_random rows of RandomState(S); strictly increasing"""
    fixed = {0, 1, 127, 128, S // 2 - 1, S // 2, S - 129, S - 128, S - 1}
    extra = np.random.RandomState(S).choice(S, n_random, replace=False)
    return tuple(sorted(fixed | {int(r) for r in extra}))


@functools.lru_cache(maxsize=None)
def many_rows(S, n=1024):
    """n rows, the most a taps call takes: rows_for(S) and random ones, row S - 1 among them"""
    have = set(rows_for(S))
    for r in np.random.RandomState(S + 1).permutation(S):
        if len(have) == n:
            break
        have.add(int(r))
    return tuple(sorted(have))


def _layer_tail64(xr, a, fp, i):
    """lc.layer64 behind the attention, on rows: LN2(x1 + ffn(x1)), x1 = LN1(x + a)"""
    f = lc._g(fp, f"ffn_blocks.{i}.")
    x1 = lc._ln64(xr + a, fp[f"norms1.{i}.weight"], fp[f"norms1.{i}.bias"])
    h = np.maximum(x1 @ f("fc1.weight").T + f("fc1.bias"), 0.0)
    return lc._ln64(x1 + h @ f("fc2.weight").T + f("fc2.bias"), fp[f"norms2.{i}.weight"], fp[f"norms2.{i}.bias"])


def rows64(x, fp, layer, rows, tail=True):
    """float64: Q (B, n, P) for the query rows `rows`, K, V (B, S, P) for all tokens, logits, probs (B, n, S), row_max,
    row_sum (B, n), ctx (B, n, P), attn64 (B, n, E) and, with tail, layer64 (B, n, E): the rows `rows` of lc.attn64 and
    lc.layer64"""
    g = lc._g(fp, f"attention_blocks.{layer}.")
    rows = list(rows)
    x = np.asarray(x, np.float64)
    lin = lambda a, n: a @ g(f"{n}_proj.weight").T + g(f"{n}_proj.bias")
    t = dict(Q=lin(x[:, rows], "q"), K=lin(x, "k"), V=lin(x, "v"))
    t["logits"] = t["Q"] @ t["K"].transpose(0, 2, 1)
    t["row_max"] = t["logits"].max(-1)
    e = np.exp(t["logits"] - t["row_max"][..., None])
    t["row_sum"] = e.sum(-1)
    t["probs"] = e / t["row_sum"][..., None]
    t["ctx"] = t["probs"] @ t["V"]
    t["attn64"] = lc.out_proj64(t["ctx"], fp, layer)
    if tail:
        t["layer64"] = _layer_tail64(x[:, rows], t["attn64"], fp, layer)
    return t


def rows32(x, twin, layer, rows, tail=True):
    """torch's CPU f32 evaluation of the same tensors under the same names: the ops of FloatTwin._attention with F.linear
    on x[:, rows] for Q, and lc.layer_torch's composition behind it; row_sum = sum(exp(s - max s)) of its own logits"""
    import torch
    F, p, a = torch.nn.functional, twin.p, f"attention_blocks.{layer}."
    E = x.shape[-1]
    with torch.no_grad():
        xt = torch.from_numpy(np.array(x, np.float32))
        xr = xt[:, list(rows)]
        lin = lambda v, n: F.linear(v, p[a + f"{n}_proj.weight"], p[a + f"{n}_proj.bias"])
        r = dict(Q=lin(xr, "q"), K=lin(xt, "k"), V=lin(xt, "v"))
        r["logits"] = torch.matmul(r["Q"], r["K"].transpose(-2, -1))
        r["row_max"] = r["logits"].max(-1).values
        r["row_sum"] = torch.exp(r["logits"] - r["row_max"][..., None]).sum(-1)
        r["probs"] = torch.softmax(r["logits"], dim=-1)
        r["ctx"] = torch.matmul(r["probs"], r["V"])
        r["attn64"] = lin(r["ctx"], "out")
        if tail:
            n = lambda v, k: F.layer_norm(v, (E,), p[f"norms{k}.{layer}.weight"], p[f"norms{k}.{layer}.bias"], 1e-5)
            x1 = n(xr + r["attn64"], 1)
            r["layer64"] = n(x1 + twin._ffn(x1, layer), 2)
        return {k: v.numpy() for k, v in r.items()}


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def ref(kind, E, S, B, layer, s=1):
    """(rows, attn64 rows, e_torch of the attention, layer64 rows, e_torch of the layer) on lc.inputs(kind, E, S, B) with
    fc.case(E, layer, s) (s = 1: the stock blob), rows = rows_for(S); the e_torch are taken on the same rows"""
    fp, _, twin = fc.case(E, layer, s)
    x = lc.inputs(kind, E, S, B)
    rows = rows_for(S)
    t, r = rows64(x, fp, layer, rows), rows32(x, twin, layer, rows)
    e = {k: float(np.abs(r[k] - t[k]).max()) for k in ("attn64", "layer64")}
    return (rows,) + _frozen(t["attn64"])[:1] + (e["attn64"],) + _frozen(t["layer64"])[:1] + (e["layer64"],)


@functools.lru_cache(maxsize=2)
def taps_ref(kind, E, S, B, layer, rows):
    """(float64, torch f32) dicts of rows64 / rows32 without the layer tail, on the stock blob"""
    fp, _, twin = lc.case(E)
    x = lc.inputs(kind, E, S, B)
    t, r = rows64(x, fp, layer, rows, tail=False), rows32(x, twin, layer, rows, tail=False)
    _frozen(*t.values(), *r.values())
    return t, r


TAP_TENSORS = ltc.TENSORS + ("logits",)


def taps_bounds(t, r):
    """long_f32_taps_common.bounds on row-sampled references: tap -> (bound, e_torch).  Q, ctx, logits, probs and row_sum
    (relative) on the sampled rows, K and V on all tokens"""
    out = {}
    for k in TAP_TENSORS:
        e = float(np.abs(r[k] - t[k]).max())
        out[k] = (3.0 * e + 4.0 * ltc.ulp32(np.abs(t[k]).max()), e)
    e = float(np.abs(r["probs"] - t["probs"]).max())
    out["probs"] = (lc.bound(e), e)
    e = float((np.abs(r["row_sum"] - t["row_sum"]) / t["row_sum"]).max())
    out["row_sum"] = (max(1e-5, 3.0 * e), e)
    return out


def taps_errors(got, t, rows):
    """long_f32_taps_common.errors on row-sampled references; got: the taps as the entry returns them (Q and ctx of all
    tokens, of which the rows `rows` are compared)"""
    rows = list(rows)
    out = {}
    for k in got:
        g = np.asarray(got[k], np.float64)
        if k in ("Q", "ctx"):
            out[k] = float(np.abs(g[:, rows] - t[k]).max())
        elif k in ("K", "V", "logits", "probs"):
            out[k] = float(np.abs(g - t[k]).max())
        elif k == "row_sum":
            out[k] = float((np.abs(g - t[k]) / t[k]).max())
    return out


# ---- wrong kernels, in float64
MUTANTS = tuple(f"{what}_{u}" for what in ("ctx", "ctx_l") for u in ("first", "middle", "last")) + ("ring_late",)


def mutants64(x, fp, layer, rows):
    """name -> the attention rows (B, n, E) a wrong flash kernel would give, restated in float64:
      ctx_<u>     the 64 keys of unit u (first, middle, last) missing from the context sum, the row sum whole
      ctx_l_<u>   the unit missing from the context sum and from the row sum
      ring_late   the K ring one slot late from unit 2 on: the logits of unit u >= 2 formed with the keys of unit u - 1
                  (V is staged apart and stays in step)"""
    t = rows64(x, fp, layer, rows, tail=False)
    S = t["K"].shape[1]
    nu = S // UNIT
    e = np.exp(t["logits"] - t["row_max"][..., None])
    out = {}
    for name, u in (("first", 0), ("middle", nu // 2), ("last", nu - 1)):
        eu = e.copy()
        eu[:, :, UNIT * u:UNIT * u + UNIT] = 0.0
        c = eu @ t["V"]
        out[f"ctx_{name}"] = lc.out_proj64(c / t["row_sum"][..., None], fp, layer)
        out[f"ctx_l_{name}"] = lc.out_proj64(c / eu.sum(-1)[..., None], fp, layer)
    K = t["K"].copy()
    K[:, 2 * UNIT:] = t["K"][:, UNIT:S - UNIT]
    s = t["Q"] @ K.transpose(0, 2, 1)
    e = np.exp(s - s.max(-1, keepdims=True))
    out["ring_late"] = lc.out_proj64((e / e.sum(-1, keepdims=True)) @ t["V"], fp, layer)
    return out


def chain32(x, fp, layer, rows):
    """an f32 model that takes no advantage of tiles: Q, K, V and the logits as numpy f32 products, e = exp(s - max s) in
    f32, then l and the context as ONE chain of S f32 additions in key order, divided at the end -> attention rows
    (B, n, E) as float64 after a float64 out_proj of the f32 context"""
    w = ltc._w(fp, layer, np.float32)
    x = np.asarray(x, np.float32)
    rows = list(rows)
    lin = lambda a, n: (a @ w[n][0].T + w[n][1]).astype(np.float32)
    Q, K, V = lin(x[:, rows], "q"), lin(x, "k"), lin(x, "v")
    s = (Q @ K.transpose(0, 2, 1)).astype(np.float32)
    e = np.exp(s - s.max(-1, keepdims=True)).astype(np.float32)
    l = np.cumsum(e, axis=-1, dtype=np.float32)[..., -1]
    c = np.empty(Q.shape, np.float32)
    for b in range(x.shape[0]):
        for i in range(len(rows)):
            c[b, i] = np.cumsum(e[b, i, :, None] * V[b], axis=0, dtype=np.float32)[-1]
    return lc.out_proj64((c / l[..., None]).astype(np.float64), fp, layer)


def unit_chain32(x, fp, layer, rows):
    """chain32 with the 64 keys of a unit added first and the S / 64 unit sums chained in order: what any kernel that
    works in tiles does, without its rescaling"""
    w = ltc._w(fp, layer, np.float32)
    x = np.asarray(x, np.float32)
    rows = list(rows)
    lin = lambda a, n: (a @ w[n][0].T + w[n][1]).astype(np.float32)
    Q, K, V = lin(x[:, rows], "q"), lin(x, "k"), lin(x, "v")
    s = (Q @ K.transpose(0, 2, 1)).astype(np.float32)
    B, n, S = s.shape
    e = np.exp(s - s.max(-1, keepdims=True)).astype(np.float32).reshape(B, n, S // UNIT, UNIT)
    l = np.cumsum(e.sum(-1, dtype=np.float32), axis=-1, dtype=np.float32)[..., -1]
    cu = np.einsum("bnuk,bukp->bnup", e, V.reshape(B, S // UNIT, UNIT, -1)).astype(np.float32)
    c = np.cumsum(cu, axis=2, dtype=np.float32)[:, :, -1]
    return lc.out_proj64((c / l[..., None]).astype(np.float64), fp, layer)


# ---- float statistics
def stats64_chunked(x, fp, layer, p_min, chunk):
    """attention_stats_f32_ref.stats64 with the S x S matrix formed `chunk` query rows at a time; the column sums add
    the chunks in order"""
    from drone_oa_iree_vit_accelerator_amd import attention_stats_f32_ref as asr
    B, S, _ = x.shape
    out = dict(col_mass=np.zeros((B, S)), col_nnz=np.zeros((B, S), np.int32))
    parts = {k: [] for k in ("row_max", "row_sum", "row_gap", "row_nnz")}
    for r0 in range(0, S, chunk):
        t = rows64(x, fp, layer, range(r0, min(r0 + chunk, S)), tail=False)
        red = asr._reduce(t["probs"], t["row_max"][..., None] - t["logits"], p_min)
        out["col_mass"] += red["col_mass"]
        out["col_nnz"] += red["col_nnz"]
        for k in parts:
            parts[k].append(red[k] if k in red else t[k])
    out.update({k: np.concatenate(v, axis=1) for k, v in parts.items()})
    return out


def stats32_chunked(x, twin, layer, chunk):
    """torch's CPU f32 col_mass and row_gap as long_f32_stats_common.refs64 forms them, `chunk` query rows at a time"""
    import torch
    B, S, _ = x.shape
    col = torch.zeros((B, S), dtype=torch.float32)
    gap = []
    for r0 in range(0, S, chunk):
        r = rows32(x, twin, layer, range(r0, min(r0 + chunk, S)), tail=False)
        lg, sm = torch.from_numpy(r["logits"]), torch.from_numpy(r["probs"])
        col += sm.sum(-2)
        gap.append((sm * (lg.max(-1, keepdim=True).values - lg)).sum(-1))
    return dict(col_mass=col.numpy(), row_gap=torch.cat(gap, dim=1).numpy())


def stats_bounds(t, r):
    """the float64 bounds of long_f32_stats_common.refs64 on any pair (float64 statistics, torch f32 statistics):
    statistic -> (bound, e_torch)"""
    out = {}
    for k in ("col_mass", "row_gap"):
        e = float(np.abs(r[k] - t[k]).max())
        out[k] = (3.0 * e + 4.0 * ltc.ulp32(np.abs(t[k]).max()), e)
    return out


@functools.lru_cache(maxsize=None)
def stats_ref(kind, E, S, s, chunk=1024):
    """(float64 statistics, bounds) of one frame lc.inputs(kind, E, S, 1) with fc.case(E, 0, s), p_min of
    long_f32_stats_common"""
    import long_f32_stats_common as lsc
    fp, _, twin = fc.case(E, 0, s)
    x = lc.inputs(kind, E, S, 1)
    t = stats64_chunked(x, fp, 0, lsc.P_MIN, chunk)
    _frozen(*t.values())
    return t, stats_bounds(t, stats32_chunked(x, twin, 0, chunk))


# ---- vocabulary frames
@functools.lru_cache(maxsize=None)
def vocabulary(S, V, singles, seed):
    """(idx (S,) the vocabulary id at every position, reps (V,) the first position of every id in increasing order,
    cls (S,) the index into reps of every position's class, counts (V,) int64 in the order of reps).  Ids 0 .. singles - 1
    occur once; every other id at least twice.  Position S - 1 holds a single, so it is a representative: the last entry
    of the taps' row table"""
    assert 0 < singles < V <= 1024 and S >= singles + 2 * (V - singles)
    rs = np.random.RandomState(seed)
    pos = rs.permutation(S)
    at = int(np.flatnonzero(pos == S - 1)[0])
    pos[0], pos[at] = pos[at], pos[0]
    idx = np.empty(S, np.int64)
    idx[pos[:singles]] = np.arange(singles)
    shared = np.concatenate([np.repeat(np.arange(singles, V), 2), rs.randint(singles, V, S - singles - 2 * (V - singles))])
    idx[pos[singles:]] = rs.permutation(shared)
    first = np.full(V, S, np.int64)
    np.minimum.at(first, idx, np.arange(S))
    order = np.argsort(first)                       # class c of reps is vocabulary id order[c]
    rank = np.empty(V, np.int64)
    rank[order] = np.arange(V)
    reps, cls = first[order], rank[idx]
    counts = np.bincount(cls, minlength=V).astype(np.int64)
    assert (counts == 1).sum() == singles and (cls[reps] == np.arange(V)).all() and reps[-1] == S - 1 and (np.diff(reps) > 0).all()
    return _frozen(idx, reps, cls, counts)


@functools.lru_cache(maxsize=None)
def vocab_f32_frame(E, S, V, singles, seed):
    """one frame (1, S, E) of V distinct lc.ln_like tokens at the positions of vocabulary(S, V, singles, seed)"""
    idx = vocabulary(S, V, singles, seed)[0]
    return _frozen(np.ascontiguousarray(lc.ln_like(1, V, E, seed)[:, idx]))[0]


@functools.lru_cache(maxsize=None)
def vocab_stats_ref(E, S, V, singles, seed, s):
    """(float64 col_mass and row_gap (1, S) of vocab_f32_frame in the class form, bounds from torch's f32 class form)
    with fc.case(E, 0, s)"""
    fp, _, twin = fc.case(E, 0, s)
    x = vocab_f32_frame(E, S, V, singles, seed)
    _, reps, cls, counts = vocabulary(S, V, singles, seed)
    t, r = rows64(x, fp, 0, reps, tail=False), rows32(x, twin, 0, reps, tail=False)
    form = lambda d, dt: dict(col_mass=(counts.astype(dt)[None, :, None] * d["probs"]).sum(1, dtype=dt),
                              row_gap=(d["probs"] * (d["row_max"][..., None] - d["logits"])).sum(-1, dtype=dt)[:, cls])
    t, r = form(t, np.float64), form(r, np.float32)
    _frozen(*t.values())
    return t, stats_bounds(t, r)


def class_stats_int8_from(rows, cls, counts):
    """attention_stats_ref.stats of one frame in the class form, from long_taps_common.mha_rows' logits and probs of one
    row per class: the row statistics spread by cls, col_mass = counts @ probs, col_nnz = counts @ (probs > 0)"""
    import long_taps_common as itc
    logits, p = rows["logits"][0], rows["probs"][0]
    row = dict(row_max=logits.max(-1).astype(np.int8), row_sum=itc.row_sums(logits).astype(np.int32),
               row_mass=p.sum(-1, dtype=np.int64).astype(np.int32), row_nnz=np.count_nonzero(p, axis=-1).astype(np.int32))
    out = {k: v[cls][None] for k, v in row.items()}
    c = counts.astype(np.float64)               # exact: every sum stays below 2^53
    out["col_mass"] = np.rint(c @ p.astype(np.float64)).astype(np.int32)[None]
    out["col_nnz"] = np.rint(c @ (p > 0).astype(np.float64)).astype(np.int32)[None]
    return _frozen_dict(out)


def _frozen_dict(d):
    _frozen(*d.values())
    return d

# ---- the int8 references at S = 65536
INT8_MODELS = (("blocks_E64_seed2_B1", 0), ("vit2l_us_E128_s1_B2", 0), ("vit2l_us_E128_s1_B2", 1))   # exact; FAST, both layers
INT8_VOCAB = (512, 256, 5)                      # V, singles, seed


def int8_vocab_frame(name, l, S):
    """(x (1, S, E) f32, reps, cls, counts): the tokens long_cases.long_f32(seed, 1, V, E, t, l) of fixture
    `name` at the positions of vocabulary(S, *INT8_VOCAB)"""
    from long_cases import long_case, long_f32
    V, singles, seed = INT8_VOCAB
    case = long_case(name)
    E, t = case.E, case.t
    idx, reps, cls, counts = vocabulary(S, V, singles, seed)
    return np.ascontiguousarray(long_f32(seed, 1, V, E, t, l)[:, idx]), reps, cls, counts


@functools.lru_cache(maxsize=None)
def int8_vocab_rows(S, n=1024):
    """(rows, at): n rows, the most a taps call takes -- the V representatives (row S - 1 among them) and random others;
    rows[at] are the representatives"""
    reps = vocabulary(S, *INT8_VOCAB)[1]
    have = {int(r) for r in reps}
    for r in np.random.RandomState(S + 2).permutation(S):
        if len(have) == min(n, S):
            break
        have.add(int(r))
    rows = np.array(sorted(have))
    return tuple(int(r) for r in rows), _frozen(np.searchsorted(rows, reps))[0]


@functools.lru_cache(maxsize=None)
def int8_vocab_ref(name, l, S=65536):
    """(x, rows, taps: logits, probs, ctx, out_q of long_taps_common.mha_rows for int8_vocab_rows(S), stats: the six
    statistics of the frame in the class form, from the representatives among those rows).  About two minutes of numpy
    at S = 65536"""
    import long_taps_common as itc
    from long_cases import long_case
    x, reps, cls, counts = int8_vocab_frame(name, l, S)
    rows, at = int8_vocab_rows(S)
    taps = dict(zip(("logits", "probs", "ctx", "out_q"), itc.mha_rows(x, long_case(name).t, list(rows), l)))
    _frozen(x, *taps.values())
    return x, rows, taps, class_stats_int8_from({k: taps[k][:, at] for k in ("logits", "probs")}, cls, counts)


def warm_int8(S=65536):
    """int8_vocab_ref of every model, side by side: numpy's integer products run one thread each"""
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(len(INT8_MODELS)) as ex:
        return list(ex.map(lambda m: int8_vocab_ref(*m, S), INT8_MODELS))
