"""CPU-side checks of the long float taps (ita_mha_long_f32_taps, Engine.mha_long_f32_taps / attention_rows_long_f32 /
attention_map_long_f32): the symbol is declared with its prototype, listed and exported, the struct is laid out as the
Python binding has it, the signatures are in place, and the code object holds the two instantiations (E = 64, 128) of each
taps kernel beside the two of each production kernel.  No compute call is made here.

The struct carries the entry's name as its TAG (an entry and a typedef of one name cannot share a C header), so the
prototype reads `const struct ita_mha_long_f32_taps* taps`; four tensor pointers, rows, n_rows and four row pointers make
ten pointer-sized slots."""
import ctypes
import inspect
import os
import re
import shutil
import tempfile

import pytest

from conftest import REPO
from drone_oa_iree_vit_accelerator_amd import host

LLVM = "/opt/rocm/lib/llvm/bin"


@pytest.fixture(scope="module")
def so():
    return host.build_extension()


def _header():
    hdr = open(os.path.join(REPO, "include", "ita_mi355x.h")).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_symbol_declared_listed_and_exported(so):
    hdr = _header()
    assert re.search(r"\bint\s+ita_mha_long_f32_taps\s*\(\s*ita_handle\s+h\s*,\s*int\s+layer\s*,\s*const\s+float\s*\*\s*x_dev\s*,"
                     r"\s*float\s*\*\s*y_dev\s*,\s*int\s+batch\s*,\s*int\s+seq_len\s*,\s*const\s+struct\s+ita_mha_long_f32_taps\s*\*\s*taps\s*,"
                     r"\s*void\s*\*\s*stream\s*\)", hdr)
    m = re.search(r"struct\s+ita_mha_long_f32_taps\s*\{(.*?)\}\s*;", hdr, flags=re.S)
    assert m, "struct ita_mha_long_f32_taps is not declared"
    body = re.sub(r"\s+", " ", m.group(1)).strip()
    want = "float *Q, *K, *V, *ctx; const int* rows; int n_rows; float *logits, *probs; float *row_max, *row_sum;"
    assert body == want, body
    assert "ita_mha_long_f32_taps" in host.EXPORTED_SYMBOLS
    lib = ctypes.CDLL(so)
    assert hasattr(lib, "ita_mha_long_f32_taps")
    assert lib.ita_abi_version() == 1
    # the int8 sibling's refusal of a float layer keeps its words
    src = open(os.path.join(REPO, "drone-oa-iree-vit-accelerator_amd", "csrc", "ita_plugin.hip")).read()
    assert "no row probabilities" in src


def test_binding_matches_the_struct():
    names = [n for n, _ in host._MhaLongF32Taps._fields_]
    assert names == ["Q", "K", "V", "ctx", "rows", "n_rows", "logits", "probs", "row_max", "row_sum"]
    p = ctypes.sizeof(ctypes.c_void_p)
    T = host._MhaLongF32Taps
    assert [getattr(T, n).offset for n in names] == [0, p, 2 * p, 3 * p, 4 * p, 5 * p, 6 * p, 7 * p, 8 * p, 9 * p]
    assert ctypes.sizeof(T) == 10 * p
    assert host.LONG_F32_TENSOR_TAPS == ("Q", "K", "V", "ctx")
    assert host.LONG_ROW_TAPS == ("logits", "probs", "row_max", "row_sum") and host.LONG_MAX_ROWS == 1024


def test_python_signatures():
    sig = inspect.signature(host.Engine.mha_long_f32_taps)
    assert list(sig.parameters) == ["self", "x", "rows", "layer"]
    assert sig.parameters["rows"].default == () and sig.parameters["layer"].default == 0
    sig = inspect.signature(host.Engine.attention_rows_long_f32)
    assert list(sig.parameters) == ["self", "x", "rows", "layer"] and sig.parameters["layer"].default == 0
    sig = inspect.signature(host.Engine.attention_map_long_f32)
    assert list(sig.parameters) == ["self", "frames", "tok_h", "tok_w", "queries", "layer", "depth_scale"]
    assert sig.parameters["layer"].default == 0 and sig.parameters["depth_scale"].default is None
    # and the entries they sit beside keep their own
    assert list(inspect.signature(host.Engine.mha_long_f32).parameters) == ["self", "x", "layer"]
    assert list(inspect.signature(host.Engine.attention_map_long).parameters) == \
        ["self", "frames", "tok_h", "tok_w", "queries", "layer", "depth_scale"]


def test_taps_kernels_in_the_code_object(so):
    """two instantiations (E = 64, 128) of each taps kernel: 512 threads, at most 256 registers, no spill and no scratch
    (LDS is dynamic: ItaLongF32Lds::TOTAL at the launch, as for the production kernel); the production kernels keep
    their two each"""
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

    def named(kernel):
        pat = r"\.name:\s+(_Z\d+%sI\S+)" % kernel
        return [(re.search(pat, b).group(1), b) for b in blocks if re.search(pat, b)]

    def field(b, name):
        return int(re.search(r"\.%s:\s+(\d+)" % name, b).group(1))

    for kernel in ("ita_lf32_proj_taps_kernel", "ita_lf32_attn_taps_kernel"):
        got = named(kernel)
        assert len(got) == 2, f"{kernel}: {[n for n, _ in got]}"
        assert {re.search(r"ILi(\d+)E", n).group(1) for n, _ in got} == {"64", "128"}
        for name, b in got:
            assert field(b, "max_flat_workgroup_size") == 512, name
            assert field(b, "vgpr_count") <= 256 and field(b, "private_segment_fixed_size") == 0, name
            assert field(b, "vgpr_spill_count") == 0, name
    for kernel in ("ita_lf32_proj_kernel", "ita_lf32_attn_kernel"):
        got = named(kernel)
        assert len(got) == 2, kernel
        for name, b in got:
            assert field(b, "private_segment_fixed_size") == 0 and field(b, "vgpr_count") <= 256, name
