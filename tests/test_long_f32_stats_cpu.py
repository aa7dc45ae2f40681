"""CPU-side checks of the long float statistics (ita_mha_long_f32_stats, Engine.attention_stats_long_f32 /
attention_received_long_f32 / attention_received_map_long_f32): the ABI (prototype, struct, export, binding,
signatures), the two kernels in the code object, the float64 definition attention_stats_f32_ref.stats64 against sums
taken directly from long_f32_taps_common.refs' probabilities, the f32 model of the kernel's two sweeps and addition order
(long_f32_stats_common.sweeps) against stats_from_taps and the bounds of the GPU test on every case of that test, six
wrong kernels those bounds must reject, and the argument refusals the entry makes before it touches its handle.
No compute call is made here.

The struct carries the entry's name as its TAG, as struct ita_mha_long_f32_taps does (an entry and a typedef of one name
cannot share a C header), so the prototype reads `const struct ita_mha_long_f32_stats* stats`."""
import ctypes
import inspect
import os
import re
import shutil
import tempfile

import numpy as np
import pytest

from conftest import REPO
from drone_oa_iree_vit_accelerator_amd import attention_stats_f32_ref as asr
from drone_oa_iree_vit_accelerator_amd import host
import long_f32_stats_common as sc
import long_f32_taps_common as ltc

LLVM = "/opt/rocm/lib/llvm/bin"
STATS = ("row_max", "row_sum", "row_gap", "row_nnz", "col_mass", "col_nnz")


@pytest.fixture(scope="module")
def so():
    return host.build_extension()


def _header():
    hdr = open(os.path.join(REPO, "include", "ita_mi355x.h")).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_symbol_declared_listed_and_exported(so):
    hdr = _header()
    assert re.search(r"\bint\s+ita_mha_long_f32_stats\s*\(\s*ita_handle\s+h\s*,\s*int\s+layer\s*,\s*const\s+float\s*\*\s*x_dev\s*,"
                     r"\s*int\s+batch\s*,\s*int\s+seq_len\s*,\s*float\s+p_min\s*,\s*const\s+struct\s+ita_mha_long_f32_stats\s*\*\s*stats\s*,"
                     r"\s*void\s*\*\s*stream\s*\)", hdr)
    m = re.search(r"struct\s+ita_mha_long_f32_stats\s*\{(.*?)\}\s*;", hdr, flags=re.S)
    assert m, "struct ita_mha_long_f32_stats is not declared"
    body = re.sub(r"\s+", " ", m.group(1)).strip()
    assert body == "float* row_max; float* row_sum; float* row_gap; int* row_nnz; float* col_mass; int* col_nnz;", body
    assert "ita_mha_long_f32_stats" in host.EXPORTED_SYMBOLS
    lib = ctypes.CDLL(so)
    assert hasattr(lib, "ita_mha_long_f32_stats")
    assert lib.ita_abi_version() == 1


def test_binding_matches_the_struct():
    assert host.LONG_F32_STATS == STATS == asr.NAMES == sc.STATS
    assert [n for n, _ in host._MhaLongF32Stats._fields_] == list(STATS)
    p = ctypes.sizeof(ctypes.c_void_p)
    for i, n in enumerate(STATS):
        assert getattr(host._MhaLongF32Stats, n).offset == i * p, n
    assert ctypes.sizeof(host._MhaLongF32Stats) == 6 * p
    # the int8 sibling keeps its own
    assert host.LONG_STATS == ("row_max", "row_sum", "row_mass", "row_nnz", "col_mass", "col_nnz")


def test_python_signatures():
    sig = inspect.signature(host.Engine.attention_stats_long_f32)
    assert list(sig.parameters) == ["self", "x", "layer", "p_min"]
    assert sig.parameters["layer"].default == 0 and sig.parameters["p_min"].default == 1.0 / 256
    sig = inspect.signature(host.Engine.attention_received_long_f32)
    assert list(sig.parameters) == ["self", "x", "layer"] and sig.parameters["layer"].default == 0
    sig = inspect.signature(host.Engine.attention_received_map_long_f32)
    assert list(sig.parameters) == ["self", "frames", "tok_h", "tok_w", "layer", "depth_scale"]
    assert sig.parameters["layer"].default == 0 and sig.parameters["depth_scale"].default is None
    assert list(inspect.signature(host.Engine._long_f32_stats).parameters) == ["self", "x", "layer", "want", "p_min"]
    assert asr.P_MIN == sc.P_MIN == 1.0 / 256


def test_kernels_in_the_code_object(so):
    """ita_lf32_stats_kernel: exactly two instantiations (E = 64, 128), 512 threads, at most 256 registers, no spill and
    no scratch (LDS is dynamic: ItaLongF32Lds::TOTAL at the launch); ita_lf32_colsum_kernel: present, no scratch"""
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

    def field(b, name):
        return int(re.search(r"\.%s:\s+(\d+)" % name, b).group(1))

    pat = r"\.name:\s+(_Z\d+ita_lf32_stats_kernelI\S+)"
    got = [(re.search(pat, b).group(1), b) for b in blocks if re.search(pat, b)]
    assert len(got) == 2, [n for n, _ in got]
    assert {re.search(r"ILi(\d+)E", n).group(1) for n, _ in got} == {"64", "128"}
    for name, b in got:
        assert field(b, "max_flat_workgroup_size") == 512, name
        assert field(b, "vgpr_count") <= 256 and field(b, "private_segment_fixed_size") == 0, name
        assert field(b, "vgpr_spill_count") == 0 and field(b, "sgpr_spill_count") == 0, name
    col = [b for b in blocks if re.search(r"\.name:\s+_Z\d+ita_lf32_colsum_kernel[A-Z]", b)]
    assert len(col) == 1
    assert field(col[0], "private_segment_fixed_size") == 0 and field(col[0], "vgpr_spill_count") == 0


@pytest.mark.parametrize("E", [64, 128])
@pytest.mark.parametrize("S,B", [(128, 3), (256, 2)])
def test_stats64_against_brute_force(E, S, B):
    """the float64 definition against sums taken from the S x S float64 probabilities of long_f32_taps_common.refs"""
    fp, _ = sc.case("plain", E)
    t, _ = ltc.refs("plain", E, S, B)
    p, lg = t["probs"], t["logits"]
    got = asr.stats64(sc.inputs("plain", E, S, B), fp, 0, sc.P_MIN)
    assert set(got) == set(STATS) | {"row_entropy"}
    for k in got:
        assert got[k].shape == (B, S) and got[k].dtype == (np.int32 if k.endswith("_nnz") else np.float64), k
    np.testing.assert_allclose(got["row_max"], lg.max(-1), rtol=1e-12)
    np.testing.assert_allclose(got["row_sum"], t["row_sum"], rtol=1e-12)
    np.testing.assert_allclose(got["col_mass"], p.sum(1), rtol=1e-12)
    np.testing.assert_array_equal(got["row_nnz"], (p >= sc.P_MIN).sum(-1))
    np.testing.assert_array_equal(got["col_nnz"], (p >= sc.P_MIN).sum(1))
    assert got["row_nnz"].sum() == got["col_nnz"].sum()
    assert (np.abs(got["col_mass"].sum(-1) - S) <= 1e-9 * S).all()
    assert (got["row_gap"] >= 0).all()
    assert (got["row_entropy"] >= -1e-12).all() and (got["row_entropy"] <= np.log(S) + 1e-12).all()
    with np.errstate(divide="ignore", invalid="ignore"):
        brute = -np.where(p > 0, p * np.log(p), 0.0).sum(-1)
    np.testing.assert_allclose(got["row_entropy"], brute, rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("E", [64, 128])
@pytest.mark.parametrize("kind,S,B", sc.CASES)
def test_model_of_the_kernel_stays_inside_both_bounds(kind, S, B, E):
    """the f32 model of the two sweeps: stats_from_taps of its own taps accepts it at the derived bounds, and it stays
    within 3 e_torch + 4 ulp of float64 -- the inputs of the GPU test are fit for both checks"""
    s, got = sc.emulated(kind, E, S, B)
    ref = asr.stats_from_taps(s, got["row_max"], got["row_sum"], sc.P_MIN)
    assert sc.compare(got, ref, S) == []
    assert (ref["row_gap"] >= 0).all() and (got["row_gap"] >= 0).all()
    ratios = sc.ratios64(got, kind, E, S, B)
    print(f"{kind} E={E} S={S} B={B}: worst error / bound against float64 {ratios}")
    assert max(ratios.values()) <= 1.0, ratios
    # a frame's column masses add up to S, to the f32 sums' accuracy
    assert (np.abs(got["col_mass"].astype(np.float64).sum(-1) - S) <= 1e-4 * S).all()
    if kind == "flat":
        assert np.median(got["row_nnz"]) >= 8          # many keys above p_min: what the case is for
    if kind == "spike_last":
        assert (got["col_mass"][:, S - 1] > S / 8).all() and (got["row_gap"] < 1e-6).mean() > 0.1


@pytest.mark.parametrize("mutation", sc.MUTATIONS)
def test_bounds_reject_a_wrong_kernel(mutation):
    S, B, E = 256, 2, 64
    s, good = sc.emulated("ramp", E, S, B)
    ref = asr.stats_from_taps(s, good["row_max"], good["row_sum"], sc.P_MIN)
    bad = sc.compare(sc.sweeps(s, sc.P_MIN, mutation), ref, S)
    assert bad, mutation
    touched = {"max_at_unit": ("row_gap", "col_mass"), "wave_missing": ("col_mass", "col_nnz"), "lane_missing": ("row_gap",),
               "last_tile": ("col_mass", "col_nnz"), "unit_swapped": ("col_mass", "col_nnz")}[mutation]
    for k in touched:
        assert any(line.startswith(k) for line in bad), (mutation, k, bad)


def test_boundary_value_counts_at_p_min():
    """rows with two equal largest logits: p = 0.5 = p_min exactly, in every row and every column twice"""
    s = sc.tie_logits(256)
    good = sc.sweeps(s, 0.5)
    ref = asr.stats_from_taps(s, good["row_max"], good["row_sum"], 0.5)
    assert (ref["probs"] == np.float32(0.5)).sum() == 2 * 256 and (ref["row_sum"] == np.float32(2.0)).all()
    assert (ref["row_nnz"] == 2).all() and (ref["col_nnz"] == 2).all()
    assert sc.compare(good, ref, 256) == []
    bad = sc.compare(sc.sweeps(s, 0.5, "gt"), ref, 256)
    assert any(line.startswith("row_nnz") for line in bad) and any(line.startswith("col_nnz") for line in bad), bad


def test_expf_shares_the_clamped_call():
    a = np.array([-400.0, -87.0, -86.99999, -3.5, 0.0, 1.25], np.float32)
    np.testing.assert_array_equal(asr.expf(a).view(np.int32), ltc.expf(a).view(np.int32))


def test_entry_refuses_bad_arguments_without_a_gpu():
    """ita_mha_long_f32_stats judges its pointers, the alignment and p_min before it uses its handle or makes a HIP call:
    a null handle, and -- behind a non-null stand-in handle that is never dereferenced -- each argument rule of the
    header.  (A call with VALID arguments is not made: it would go on to the GPU.)"""
    host.build_extension()
    L = host.lib()
    INVALID = -1
    fake_handle = ctypes.create_string_buffer(1 << 16)
    x, out = ctypes.create_string_buffer(64), ctypes.create_string_buffer(64)
    o = ctypes.addressof(out)
    full = dict(row_max=o, row_sum=o + 4, row_gap=o + 8, row_nnz=o + 12, col_mass=o + 16, col_nnz=o + 20)

    def call(h=ctypes.addressof(fake_handle), xp=ctypes.addressof(x), p_min=1.0 / 256, st=full):
        s = None if st is None else ctypes.byref(host._MhaLongF32Stats(**st))
        return L.ita_mha_long_f32_stats(h, 0, xp, 1, 128, p_min, s, None)

    bad = [dict(h=None), dict(xp=None), dict(st=None), dict(st={})]
    bad += [dict(st=dict(full, **{k: full[k] + 2})) for k in STATS] + [dict(st={"col_mass": o + 1})]
    bad += [dict(p_min=v) for v in (0.0, -1.0, 1.5, float("nan"), float("inf"))]
    for kw in bad:
        assert call(**kw) == INVALID, kw
        assert L.ita_last_error() == INVALID and L.ita_error_string()
    assert not any(out.raw)
