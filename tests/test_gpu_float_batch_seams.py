"""The float kernels past one frame / one tile per workgroup on the MI355X.

ita_attn_f32_kernel<E> runs min(B, CUs) workgroups over frames and ita_ffn_f32_kernel<E> min(4 B, 2 CUs) workgroups over
32-token tiles, both in a grid stride.  Below B = CUs / 2 every workgroup sees one tile, below B = CUs one frame: the later
iterations -- the barriers that protect the x tile, the K / V image and the x1 / hidden / output tiles from the next
iteration, the register prefetch of the next x1 tile, the f16 plane stores, the y == nullptr form and the h0 side copy of
a walked tile loop -- run here.

Batches, from the CU count of the device (256 on an MI355X):
  B0 = CUs // 2 + 1   FFN: more tiles than workgroups, the first workgroups take two; attention: one frame each
  B1 = CUs + 1        FFN: every workgroup two tiles or three;                       attention: workgroup 0 takes two frames
  B2 = 2 CUs + 3      FFN: four or five tiles;                                       attention: workgroups 0..2 take three
Reference: the same frames in consecutive chunks of at most 32 (one frame, at most one tile per workgroup: the regime the
other tests hold to float64 and to the oracle), compared bit for bit over every frame; ita_ffn_f32 is anchored to the
oracle composition on 8 frames per batch.  A failure names the first differing frame and its place in each kernel's grid.

Blob families: ITAW0003 E = 64 (one layer, fusion tail), ITAW0003 E = 128 (two layers, no tail), ITAW0002 E = 64 (int8
attention in front of the float FFN)."""
import numpy as np
import pytest

from drone_oa_iree_vit_accelerator_amd import host, synth
from gpu_support import cu
from float_graph_common import ln_like, setup_float, setup_notail, unpack
from only_attn_common import setup_only_attn

pytestmark = pytest.mark.gpu

CHUNK = 32
FAMILIES = ("itaw3_e64", "itaw3_e128", "itaw2_e64")
FLOAT_ATTN = ("itaw3_e64", "itaw3_e128")


def _family(name):
    """(blob, E, layers)"""
    if name == "itaw3_e64":
        return setup_float(1)[2], 64, 1
    if name == "itaw3_e128":
        _, _, blob, L = setup_notail(128)
        return blob, 128, L
    return setup_only_attn(1)[2], 64, 1


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _iters(items, grid):
    """(fewest, most) loop iterations of a workgroup when `items` are walked by `grid` workgroups in a grid stride"""
    return items // grid, -(-items // grid)


def _batches():
    """(B0, B1, B2), with the iteration counts they stand for asserted"""
    cus = _cus()
    B0, B1, B2 = cus // 2 + 1, cus + 1, 2 * cus + 3
    attn = lambda B: _iters(B, min(B, cus))
    ffn = lambda B: _iters(4 * B, min(4 * B, 2 * cus))
    assert attn(B0) == (1, 1) and ffn(B0) == (1, 2) and 0 < 4 * B0 - 2 * cus <= 4
    assert attn(B1) == (1, 2) and B1 - cus == 1 and ffn(B1) == (2, 3)
    assert attn(B2) == (2, 3) and B2 - 2 * cus == 3 and ffn(B2) == (4, 5)
    assert attn(CHUNK) == (1, 1) and ffn(CHUNK) == (1, 1)   # the reference's chunks: one frame, one tile per workgroup
    return B0, B1, B2


def _chunked(fn, x):
    """fn over consecutive chunks of at most CHUNK frames of x, joined"""
    return np.concatenate([fn(np.ascontiguousarray(x[i:i + CHUNK])) for i in range(0, x.shape[0], CHUNK)])


def _assert_frames_equal(got, want, what, frame_axis=0, tokens=True):
    """bit-equality over every frame; on failure the first differing frame (and 32-token tile) and where each kernel's
    grid stride puts it: index % grid = the workgroup, index // grid = its loop iteration"""
    got, want = np.moveaxis(np.asarray(got), frame_axis, 0), np.moveaxis(np.asarray(want), frame_axis, 0)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if np.array_equal(got, want):
        return
    B, cus = got.shape[0], _cus()
    ne = got != want
    bad = np.flatnonzero(ne.reshape(B, -1).any(1))
    f = int(bad[0])
    ga, gf = min(B, cus), min(4 * B, 2 * cus)
    msg = (f"{what}: {bad.size} of {B} frames differ from the chunked run; first frame {f}: attention grid {ga}, "
           f"workgroup {f % ga}, iteration {f // ga}")
    if tokens:
        tok = int(np.flatnonzero(ne[f].reshape(128, -1).any(1))[0])
        tile = 4 * f + tok // 32
        msg += f"; first token {tok} = tile {tile}: FFN grid {gf}, workgroup {tile % gf}, iteration {tile // gf}"
    else:
        msg += f"; tiles {4 * f}..{4 * f + 3}: FFN grid {gf}, workgroups {4 * f % gf}.., iteration {4 * f // gf}"
    raise AssertionError(msg + f"; max |diff| {np.nanmax(np.abs(got[f].astype(np.float64) - want[f])):.3e}")


def _pick8(B):
    """8 frames: the first, the last, and, where the batch has them, frames of the second and third pass of a CUs-frame
    grid (the attention's; the FFN's grid holds CUs / 2 frames, so these are its third and later passes)"""
    cus = _cus()
    want = [0, B - 1, cus + 7, 2 * cus, cus, 2 * cus - 1, cus // 2 + 3, B - 2, 1, B // 2, B // 3, B // 4, 2, 3]
    pick = []
    for f in want:
        if 0 <= f < B and f not in pick:
            pick.append(f)
    return np.array(sorted(pick[:8]))


# ---- ita_mha_f32
@pytest.mark.parametrize("family", FLOAT_ATTN)
def test_mha_f32_past_one_frame_per_workgroup(family):
    blob, E, L = _family(family)
    _, B1, B2 = _batches()
    eng = host.Engine(blob, device=0)
    for B in (B1, B2):
        x = ln_like(B, 100 + B, E)
        for l in range(L):
            run = lambda a: eng.mha_f32(cu(a), l).cpu().numpy()
            _assert_frames_equal(run(x), _chunked(run, x), f"mha_f32 {family} B={B} layer {l}")
    eng.close()


# ---- ita_ffn_f32
@pytest.mark.parametrize("family", FAMILIES)
def test_ffn_f32_past_one_tile_per_workgroup(oracle, family):
    blob, E, L = _family(family)
    t = unpack(blob)
    eng = host.Engine(blob, device=0)
    for B in _batches():
        x = ln_like(B, 200 + B, E)
        x[0, 0, :8] = 0.0
        pick = _pick8(B)
        assert pick.size == 8 and pick[0] == 0 and pick[-1] == B - 1
        if B == _batches()[2]:
            assert ((pick >= _cus()) & (pick < 2 * _cus())).any() and (pick >= 2 * _cus()).any()
        for l in range(L):
            run = lambda a: eng.ffn_f32(cu(a), l).cpu().numpy()
            y = run(x)
            _assert_frames_equal(y, _chunked(run, x), f"ffn_f32 {family} B={B} layer {l}")
            hid = np.maximum(oracle.linear_f32(x[pick], t[f"ffn{l}.w1f"], t[f"ffn{l}.b1f"]), np.float32(0))
            want = oracle.linear_f32(hid, t[f"ffn{l}.w2f"], t[f"ffn{l}.b2f"])
            np.testing.assert_array_equal(y[pick], want, err_msg=f"ffn_f32 {family} B={B} layer {l} frames {pick.tolist()} against the oracle")
    eng.close()


# ---- ita_encoder_layer: attention + LN1 into the workspace, FFN + LN2
@pytest.mark.parametrize("family", FAMILIES)
def test_encoder_layer_past_one_frame_per_workgroup(family):
    blob, E, L = _family(family)
    B0, B1, B2 = _batches()
    eng = host.Engine(blob, device=0)
    for B in (B0, B1, B2):
        x = ln_like(B, 300 + B, E)
        for l in range(L):
            run = lambda a: eng.encoder_layer(cu(a), l).cpu().numpy()
            want = _chunked(run, x)
            _assert_frames_equal(run(x), want, f"encoder_layer {family} B={B} layer {l}")
            if B == B2:   # in place: y aliases x across the iterations
                xx = cu(x)
                host._chk(host.lib().ita_encoder_layer(eng._h, l, xx.data_ptr(), xx.data_ptr(), B, host._stream_ptr(eng.device)))
                _assert_frames_equal(xx.cpu().numpy(), want, f"encoder_layer in place {family} B={B} layer {l}")
    eng.close()


# ---- the whole forward
def _step_inputs(seed, B, NS=None):
    fr = synth.frames(seed, B)
    rs = np.random.RandomState(seed)
    h0 = (0.3 * rs.standard_normal((3, NS or B, 128))).astype(np.float32)
    c0 = (0.3 * rs.standard_normal((3, NS or B, 128))).astype(np.float32)
    return fr["img_u8"], fr["desvel"], fr["quat"], h0, c0


@pytest.mark.parametrize("family", FAMILIES)
def test_forward_past_one_frame_per_workgroup(family):
    """taps x1 / x2, vel, h, c equal the chunked runs in both tail modes; without taps (mode 1: the FFN of the last layer
    writes the f16 planes only, y == nullptr) the same vel, h, c"""
    import torch
    blob = _family(family)[0]
    _, B1, _ = _batches()
    eng = host.Engine(blob, device=0)
    img, dv, qt, h0, c0 = _step_inputs(31, B1)

    def run(img, dv, qt, h0, c0):
        v, (h, c), tp = eng.forward(cu(img), cu(dv), cu(qt), (cu(h0), cu(c0)), taps=True)
        torch.cuda.synchronize()
        return dict(vel=v.cpu().numpy(), h=h.cpu().numpy(), c=c.cpu().numpy(), x1=tp["x1"].cpu().numpy(), x2=tp["x2"].cpu().numpy())

    for mode in (0, 1):
        eng.set_tail_mode(mode)
        got = run(img, dv, qt, h0, c0)
        parts = [run(img[i:i + CHUNK], dv[i:i + CHUNK], qt[i:i + CHUNK], np.ascontiguousarray(h0[:, i:i + CHUNK]),
                     np.ascontiguousarray(c0[:, i:i + CHUNK])) for i in range(0, B1, CHUNK)]
        for k in ("x1", "x2", "vel", "h", "c"):
            ax = 1 if k in ("h", "c") else 0
            want = np.concatenate([p[k] for p in parts], axis=ax)
            _assert_frames_equal(got[k], want, f"forward {family} tail mode {mode} B={B1}: {k}", frame_axis=ax, tokens=k in ("x1", "x2"))
        v, (h, c) = eng.forward(cu(img), cu(dv), cu(qt), (cu(h0), cu(c0)))
        for k, g in (("vel", v), ("h", h), ("c", c)):
            _assert_frames_equal(g.cpu().numpy(), got[k], f"forward without taps {family} tail mode {mode} B={B1}: {k}",
                                 frame_axis=1 if k != "vel" else 0, tokens=False)
    eng.close()


@pytest.mark.parametrize("family", FAMILIES)
def test_forward_slots_past_one_frame_per_workgroup(family):
    """the state gathered through a random permutation of slots (the FFN's h0 side copy walks it tile after tile): vel and
    the scattered state equal the eager forward on the gathered state; rows that no slot names stay as they were"""
    import torch
    blob = _family(family)[0]
    _, B1, _ = _batches()
    NS = B1 + 5
    eng = host.Engine(blob, device=0)
    img, dv, qt, h0, c0 = _step_inputs(47, B1, NS)
    perm = np.random.RandomState(B1).permutation(NS)
    slots, rest = perm[:B1].astype(np.int32), np.sort(perm[B1:])
    assert rest.size == 5 and not (slots == np.arange(B1)).all()
    sh, sc = cu(h0.copy()), cu(c0.copy())
    vel = eng.forward_slots(cu(img), cu(dv), cu(qt), sh, sc, cu(slots))
    v2, (h2, c2) = eng.forward(cu(img), cu(dv), cu(qt), (cu(h0[:, slots]), cu(c0[:, slots])))
    torch.cuda.synchronize()
    _assert_frames_equal(vel.cpu().numpy(), v2.cpu().numpy(), f"forward_slots {family} B={B1}: vel", tokens=False)
    sh, sc = sh.cpu().numpy(), sc.cpu().numpy()
    _assert_frames_equal(sh[:, slots], h2.cpu().numpy(), f"forward_slots {family} B={B1}: h", frame_axis=1, tokens=False)
    _assert_frames_equal(sc[:, slots], c2.cpu().numpy(), f"forward_slots {family} B={B1}: c", frame_axis=1, tokens=False)
    assert np.array_equal(sh[:, rest], h0[:, rest]) and np.array_equal(sc[:, rest], c0[:, rest])
    eng.close()


@pytest.mark.parametrize("family", FAMILIES)
def test_graphed_step_past_one_frame_per_workgroup(family):
    import torch
    blob = _family(family)[0]
    _, B1, _ = _batches()
    eng = host.Engine(blob, device=0)
    g = eng.graphed_step(B1)
    st = (torch.zeros((3, B1, 128), device="cuda"), torch.zeros((3, B1, 128), device="cuda"))
    for t in range(3):
        fr = synth.frames(600 + t, B1)
        img, dv, qt = cu(fr["img_u8"]), cu(fr["desvel"]), cu(fr["quat"])
        g.img.copy_(img); g.desvel.copy_(dv.reshape(B1)); g.quat.copy_(qt)
        vg = g().clone()
        ve, st = eng.forward(img, dv, qt, st)
        torch.cuda.synchronize()
        _assert_frames_equal(vg.cpu().numpy(), ve.cpu().numpy(), f"graphed step {family} B={B1} replay {t}: vel", tokens=False)
        _assert_frames_equal(g.h.cpu().numpy(), st[0].cpu().numpy(), f"graphed step {family} B={B1} replay {t}: h", frame_axis=1, tokens=False)
        _assert_frames_equal(g.c.cpu().numpy(), st[1].cpu().numpy(), f"graphed step {family} B={B1} replay {t}: c", frame_axis=1, tokens=False)
    del g
    eng.close()
