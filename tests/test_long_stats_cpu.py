"""CPU-side checks of the long-sequence statistics (ita_mha_long_int8_stats, Engine.attention_stats_long /
attention_received_long / attention_received_map_long): the numpy definition attention_stats_ref against sums taken
directly from mha_heads_ref.mha's probabilities, its closed form on the crafted frames of long_taps_common, and the ABI:
prototype, struct, export, binding, signatures, and the two instantiations of ita_long_stats_kernel in the code object.
No compute call is made here."""
import ctypes
import inspect
import os
import re
import shutil
import tempfile

import numpy as np
import pytest

from conftest import REPO
from drone_oa_iree_vit_accelerator_amd import attention_stats_ref as asr
from drone_oa_iree_vit_accelerator_amd import host
from drone_oa_iree_vit_accelerator_amd import mha_heads_ref as ref
import long_taps_common as ltc
from long_cases import long_case, tokens

LLVM = "/opt/rocm/lib/llvm/bin"
STATS = ("row_max", "row_sum", "row_mass", "row_nnz", "col_mass", "col_nnz")


@pytest.mark.parametrize("name", ["vitlstm_E64_seed0_B2", "blocks_E128_seed0_B1"])
def test_stats_are_the_sums_of_the_definitions_probabilities(name):
    S, B = 256, 2
    case = long_case(name)
    E, t = case.E, case.t
    x = tokens(S + B, B, S, E, t)
    _, tp = ref.mha(x, t, 1, 0)
    p, lg = tp["probs"].astype(np.int64), tp["logits"]
    for block in (512, 96):          # one block, and blocks that do not divide S
        got = asr.stats(x, t, 0, block=block)
        assert tuple(got) == STATS
        for k in STATS:
            assert got[k].shape == (B, S) and got[k].dtype == (np.int8 if k == "row_max" else np.int32), k
        np.testing.assert_array_equal(got["row_max"], lg.max(-1))
        np.testing.assert_array_equal(got["row_sum"], ltc.row_sums(lg))
        np.testing.assert_array_equal(got["row_mass"], p.sum(-1))
        np.testing.assert_array_equal(got["row_nnz"], (p > 0).sum(-1))
        np.testing.assert_array_equal(got["col_mass"], p.sum(1))
        np.testing.assert_array_equal(got["col_nnz"], (p > 0).sum(1))
        np.testing.assert_array_equal(got["row_mass"].sum(-1), got["col_mass"].sum(-1))
        np.testing.assert_array_equal(got["row_nnz"].sum(-1), got["col_nnz"].sum(-1))
    assert got["row_mass"].max() > 0 and got["col_nnz"].max() > 1


@pytest.mark.parametrize("form", ["fast", "exact"])
def test_closed_form_on_crafted_frames(form):
    d = ltc.fixture()
    _, t, _ = ltc.crafted(form)
    x = ltc.frames_for(form, d["x256"][:4])
    got = asr.stats(x, t)
    for b in range(4):
        want = asr.stats_from_row(d["y256"][b], 256)
        assert set(want) == {"row_mass", "row_nnz", "col_mass", "col_nnz"}
        for k, v in want.items():
            assert v.dtype == np.int32 and v.shape == (256,)
            np.testing.assert_array_equal(got[k][b], v, err_msg=f"{form} frame {b} {k}")
        np.testing.assert_array_equal(got["row_max"][b], np.full(256, d["x256"][b].max()))
        np.testing.assert_array_equal(got["row_sum"][b], np.full(256, ltc.row_sums(d["x256"][b])))


@pytest.fixture(scope="module")
def so():
    return host.build_extension()


def _header():
    hdr = open(os.path.join(REPO, "include", "ita_mi355x.h")).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_symbol_declared_listed_and_exported(so):
    hdr = _header()
    assert re.search(r"\bint\s+ita_mha_long_int8_stats\s*\(\s*ita_handle\s+h\s*,\s*int\s+layer\s*,\s*const\s+float\s*\*\s*x_dev\s*,"
                     r"\s*int\s+batch\s*,\s*int\s+seq_len\s*,\s*const\s+ita_mha_long_stats\s*\*\s*stats\s*,\s*void\s*\*\s*stream\s*\)", hdr)
    m = re.search(r"typedef\s+struct\s+ita_mha_long_stats\s*\{(.*?)\}\s*ita_mha_long_stats\s*;", hdr, flags=re.S)
    assert m, "struct ita_mha_long_stats is not declared"
    body = re.sub(r"\s+", " ", m.group(1)).strip()
    assert body == "int8_t* row_max; int* row_sum; int* row_mass; int* row_nnz; int* col_mass; int* col_nnz;", body
    assert "ita_mha_long_int8_stats" in host.EXPORTED_SYMBOLS
    lib = ctypes.CDLL(so)
    assert hasattr(lib, "ita_mha_long_int8_stats")
    assert lib.ita_abi_version() == 1


def test_binding_matches_the_struct():
    assert host.LONG_STATS == STATS
    assert [n for n, _ in host._MhaLongStats._fields_] == list(STATS)
    p = ctypes.sizeof(ctypes.c_void_p)
    for i, n in enumerate(STATS):
        assert getattr(host._MhaLongStats, n).offset == i * p, n
    assert ctypes.sizeof(host._MhaLongStats) == 6 * p


def test_python_signatures():
    for fn in (host.Engine.attention_stats_long, host.Engine.attention_received_long):
        sig = inspect.signature(fn)
        assert list(sig.parameters) == ["self", "x", "layer"] and sig.parameters["layer"].default == 0
    sig = inspect.signature(host.Engine.attention_received_map_long)
    assert list(sig.parameters) == ["self", "frames", "tok_h", "tok_w", "layer", "depth_scale"]
    assert sig.parameters["layer"].default == 0 and sig.parameters["depth_scale"].default is None
    assert list(inspect.signature(host.Engine._long_stats).parameters) == ["self", "x", "layer", "want"]


def test_stats_kernel_in_the_code_object(so):
    """exactly two instantiations (FAST or not: E does not appear), 512 threads, no scratch"""
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
    pat = r"\.name:\s+(_Z\d+ita_long_stats_kernelI\S+)"
    got = [(re.search(pat, b).group(1), b) for b in blocks if re.search(pat, b)]
    assert len(got) == 2, [n for n, _ in got]
    assert {re.search(r"ILb([01])E", n).group(1) for n, _ in got} == {"0", "1"}
    for name, b in got:
        assert int(re.search(r"\.max_flat_workgroup_size:\s+(\d+)", b).group(1)) == 512, name
        assert int(re.search(r"\.vgpr_count:\s+(\d+)", b).group(1)) <= 128, name          # four waves per SIMD
        assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", b).group(1)) == 0, name
