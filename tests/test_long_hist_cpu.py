"""CPU-side checks of the long-sequence histograms (ita_mha_long_int8_hist, Engine.attention_histograms_long): the numpy
definition attention_hist_ref against counts taken directly from mha_heads_ref.mha's taps and from attention_stats_ref, its
class form against the whole matrix, the crafted clamp frames of softmax_clamp_common, the input conditions the GPU tests
rely on, and the ABI: prototype, struct, export, binding, signatures, and the two instantiations of ita_long_hist_kernel in
the code object.  No compute call is made here."""
import ctypes
import inspect
import os
import re
import shutil
import tempfile

import numpy as np
import pytest

from conftest import REPO
from drone_oa_iree_vit_accelerator_amd import attention_hist_ref as ahr
from drone_oa_iree_vit_accelerator_amd import attention_stats_ref as asr
from drone_oa_iree_vit_accelerator_amd import host
from drone_oa_iree_vit_accelerator_amd import mha_heads_ref as ref
import long_hist_common as lhc
import long_limits_common as llc
import softmax_clamp_common as scc
from long_cases import long_case, long_f32

LLVM = "/opt/rocm/lib/llvm/bin"

def _shapes(h, B):
    assert tuple(h) == lhc.NAMES
    for k in lhc.NAMES:
        assert h[k].shape == (B, lhc.WIDTH[k]) and h[k].dtype == lhc.DTYPES[k], (k, h[k].shape, h[k].dtype)


@pytest.mark.parametrize("name", ["vitlstm_E64_seed0_B2", "blocks_E128_seed0_B1"])
def test_hist_is_the_count_of_the_definitions_tensors(name):
    S, B = 256, 2
    case = long_case(name)
    E, t = case.E, case.t
    x = long_f32(S + B, B, S, E, t)
    _, tp, acc = ref.mha(x, t, 1, 0, taps=True)
    st = asr.stats(x, t)
    for block in (512, 96):          # one block, and blocks that do not divide S
        h = ahr.hist(x, t, 0, block=block)
        _shapes(h, B)
        for k in ("logits", "shifts", "probs"):
            np.testing.assert_array_equal(h[k].sum(-1), np.full(B, S * S), err_msg=k)
        v = np.arange(256)
        np.testing.assert_array_equal((h["probs"] * v).sum(-1), st["row_mass"].astype(np.int64).sum(-1))
        np.testing.assert_array_equal(S * S - h["probs"][:, 0], st["row_nnz"].astype(np.int64).sum(-1))
        lg = tp["logits"].astype(np.int64)
        for b in range(B):
            np.testing.assert_array_equal(h["logits"][b], np.bincount((lg[b] + 128).ravel(), minlength=256))
            np.testing.assert_array_equal(h["probs"][b], np.bincount(tp["probs"][b].ravel(), minlength=256))
            np.testing.assert_array_equal(h["shifts"][b], np.bincount((lg[b].max(-1, keepdims=True) - lg[b]).ravel(), minlength=256))
            assert tuple(h["acc_range"][b]) == (acc["L"][b].min(), acc["L"][b].max())


@pytest.mark.parametrize("name,l", [("vitlstm_E64_seed0_B2", 0), ("vit2l_us_E128_s1_B2", 1)])
def test_class_form_equals_the_whole_matrix(name, l):
    """an S = 512 frame drawn from 48 distinct tokens, 16 of them single"""
    S, V, singles, seed = 512, 48, 16, 9
    case = long_case(name)
    E, t = case.E, case.t
    idx, reps, cls, counts = llc.vocabulary(S, V, singles, seed)
    assert int((counts == 1).sum()) == 16 and counts.sum() == S
    x = np.ascontiguousarray(long_f32(seed, 1, 64, E, t, l)[:, :V][:, idx])    # (_long_f32 builds blocks of 32 tokens)
    want = ahr.hist(x, t, l)
    got = ahr.hist_from_classes(x[0, reps], counts, t, l)
    _shapes(got, 1)
    for k in lhc.NAMES:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    np.testing.assert_array_equal(ahr.hist_from_classes(x[:, reps], counts, t, l)["probs"], want["probs"])
    assert np.count_nonzero(want["probs"][0]) > 16


@pytest.mark.parametrize("S", lhc.CLAMP_S)
@pytest.mark.parametrize("form", lhc.CLAMP_FORMS)
def test_crafted_clamp_frames(form, S):
    """raw logits in about +-600: what the clamp changed, and the histogram of the clipped logits, from the wanted raw
    integers alone"""
    x, h, raw = lhc.clamp_expected(form, S)
    _shapes(h, 3)
    below, above = (raw < -128).sum((-2, -1)), (raw > 127).sum((-2, -1))
    np.testing.assert_array_equal(h["logits_out"], np.stack([below, above], axis=1))
    for b in range(3):
        np.testing.assert_array_equal(h["logits"][b], np.bincount((np.clip(raw[b], -128, 127) + 128).ravel(), minlength=256))
        np.testing.assert_array_equal(h["shifts"][b], np.bincount(scc.shift_definition(raw[b]).ravel(), minlength=256))
    assert 16720 <= below.min() and below.max() <= 106260, below
    assert 16764 <= above[:2].min() and above[:2].max() <= 42357 and above[2] == 0, above
    _, _, acc = ref.mha(x, scc.crafted(form)[1], 1, taps=True)
    np.testing.assert_array_equal(h["acc_range"], np.stack([acc["L"].min((1, 2, 3)), acc["L"].max((1, 2, 3))], axis=1))


@pytest.mark.parametrize("S,B", lhc.SHAPES)
@pytest.mark.parametrize("name,l", lhc.FIXTURES)
def test_input_conditions_of_the_gpu_tests(name, l, S, B):
    """a kernel that caps the shift histogram at 15, or drops a tile, is visibly wrong on these inputs"""
    _, h = lhc.expected(name, l, S, B)
    _shapes(h, B)
    lb, s32, pb = lhc.conditions(h)
    print(f"{name} layer {l} S={S}: >= {lb} logit bins, >= {100 * s32:.1f} % of shifts above 31, >= {pb} probability bins")
    for k in ("logits", "shifts", "probs"):
        np.testing.assert_array_equal(h[k].sum(-1), np.full(B, S * S), err_msg=k)


@pytest.fixture(scope="module")
def so():
    return host.build_extension()


def _header():
    hdr = open(os.path.join(REPO, "include", "ita_mi355x.h")).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_symbol_declared_listed_and_exported(so):
    hdr = _header()
    assert re.search(r"\bint\s+ita_mha_long_int8_hist\s*\(\s*ita_handle\s+h\s*,\s*int\s+layer\s*,\s*const\s+float\s*\*\s*x_dev\s*,"
                     r"\s*int\s+batch\s*,\s*int\s+seq_len\s*,\s*const\s+ita_mha_long_hist\s*\*\s*hist\s*,\s*void\s*\*\s*stream\s*\)", hdr)
    m = re.search(r"typedef\s+struct\s+ita_mha_long_hist\s*\{(.*?)\}\s*ita_mha_long_hist\s*;", hdr, flags=re.S)
    assert m, "struct ita_mha_long_hist is not declared"
    body = re.sub(r"\s+", " ", m.group(1)).strip()
    assert body == "int64_t *logits, *shifts, *probs; int64_t *logits_out; int32_t *acc_range;", body
    assert "ita_mha_long_int8_hist" in host.EXPORTED_SYMBOLS
    lib = ctypes.CDLL(so)
    assert hasattr(lib, "ita_mha_long_int8_hist")
    assert lib.ita_abi_version() == 1


def test_hist_kernel_in_the_code_object(so):
    """exactly two instantiations (FAST or not: E does not appear), 512 threads, four waves per SIMD, no scratch"""
    objdump, readelf = os.path.join(LLVM, "llvm-objdump"), os.path.join(LLVM, "llvm-readelf")
    if not (os.path.exists(objdump) and os.path.exists(readelf)):
        pytest.skip("llvm-objdump / llvm-readelf unavailable")
    with tempfile.TemporaryDirectory() as td:      # --offloading drops the extracted code objects in cwd
        cp = shutil.copy(so, td)
        out = os.popen(f"cd {td} && {objdump} --offloading {cp} 2>/dev/null").read()
        if not out:
            pytest.skip("llvm-objdump unavailable")
        cos = [os.path.join(td, f) for f in os.listdir(td) if "gfx950" in f]
        assert cos, "no gfx950 code object extracted"
        notes = "".join(os.popen(f"{readelf} --notes {c} 2>/dev/null").read() for c in cos)
    blocks = notes.split("- .agpr_count:")[1:]
    pat = r"\.name:\s+(_Z\d+ita_long_hist_kernelI\S+)"
    got = [(re.search(pat, b).group(1), b) for b in blocks if re.search(pat, b)]
    assert len(got) == 2, [n for n, _ in got]
    assert {re.search(r"ILb([01])E", n).group(1) for n, _ in got} == {"0", "1"}
    for name, b in got:
        assert int(re.search(r"\.max_flat_workgroup_size:\s+(\d+)", b).group(1)) == 512, name
        assert int(re.search(r"\.vgpr_count:\s+(\d+)", b).group(1)) <= 128, name          # four waves per SIMD
        assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", b).group(1)) == 0, name
        assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", b).group(1)) == 0, name


def test_binding_matches_the_struct():
    fields = ("logits", "shifts", "probs", "logits_out", "acc_range")
    assert set(host.LONG_HIST) == set(fields) and host.LONG_HIST == ahr.NAMES
    assert [n for n, _ in host._MhaLongHist._fields_] == list(fields)
    p = ctypes.sizeof(ctypes.c_void_p)
    for i, n in enumerate(fields):
        assert getattr(host._MhaLongHist, n).offset == i * p, n
    assert ctypes.sizeof(host._MhaLongHist) == 5 * p


def test_python_signatures():
    sig = inspect.signature(host.Engine.attention_histograms_long)
    assert list(sig.parameters) == ["self", "x", "layer", "stages"]
    assert sig.parameters["layer"].default == 0 and sig.parameters["stages"].default is False
    sig = inspect.signature(host.Engine.attention_histograms_frames_long)
    assert list(sig.parameters) == ["self", "frames", "tok_h", "tok_w", "layer", "depth_scale"]
    assert sig.parameters["layer"].default == 0 and sig.parameters["depth_scale"].default is None
