"""CPU-side checks of the long-sequence taps (ita_mha_long_int8_taps, Engine.mha_long_taps / attention_rows_long /
attention_map_long): the symbol is declared with its prototype, listed and exported, the struct is laid out as the
Python binding has it, the signatures are in place, and the code object holds the four instantiations of each taps
kernel beside the untouched eight of each production kernel.  No compute call is made here."""
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
    assert re.search(r"\bint\s+ita_mha_long_int8_taps\s*\(\s*ita_handle\s+h\s*,\s*int\s+layer\s*,\s*const\s+float\s*\*\s*x_dev\s*,"
                     r"\s*float\s*\*\s*y_dev\s*,\s*int\s+batch\s*,\s*int\s+seq_len\s*,\s*const\s+ita_mha_long_taps\s*\*\s*taps\s*,"
                     r"\s*void\s*\*\s*stream\s*\)", hdr)
    m = re.search(r"typedef\s+struct\s+ita_mha_long_taps\s*\{(.*?)\}\s*ita_mha_long_taps\s*;", hdr, flags=re.S)
    assert m, "struct ita_mha_long_taps is not declared"
    body = re.sub(r"\s+", " ", m.group(1)).strip()
    want = ("int8_t *x_q, *Q, *K, *V, *ctx, *out_q; const int* rows; int n_rows; int8_t* logits; uint8_t* probs; "
            "int8_t* row_max; int* row_sum;")
    assert body == want, body
    assert "ita_mha_long_int8_taps" in host.EXPORTED_SYMBOLS
    lib = ctypes.CDLL(so)
    assert hasattr(lib, "ita_mha_long_int8_taps")
    assert lib.ita_abi_version() == 1


def test_binding_matches_the_struct():
    names = [n for n, _ in host._MhaLongTaps._fields_]
    assert names == ["x_q", "Q", "K", "V", "ctx", "out_q", "rows", "n_rows", "logits", "probs", "row_max", "row_sum"]
    p = ctypes.sizeof(ctypes.c_void_p)
    assert host._MhaLongTaps.rows.offset == 6 * p and host._MhaLongTaps.n_rows.offset == 7 * p
    assert host._MhaLongTaps.logits.offset == 8 * p and ctypes.sizeof(host._MhaLongTaps) == 12 * p
    assert host.LONG_MAX_ROWS == 1024


def test_python_signatures():
    sig = inspect.signature(host.Engine.mha_long_taps)
    assert list(sig.parameters) == ["self", "x", "rows", "layer"]
    assert sig.parameters["rows"].default == () and sig.parameters["layer"].default == 0
    sig = inspect.signature(host.Engine.attention_rows_long)
    assert list(sig.parameters) == ["self", "x", "rows", "layer"] and sig.parameters["layer"].default == 0
    sig = inspect.signature(host.Engine.attention_map_long)
    assert list(sig.parameters) == ["self", "frames", "tok_h", "tok_w", "queries", "layer", "depth_scale"]
    assert sig.parameters["layer"].default == 0 and sig.parameters["depth_scale"].default is None
    # and the entry the taps sit beside keeps its own
    assert list(inspect.signature(host.Engine.mha_long).parameters) == ["self", "x", "layer"]


def test_taps_kernels_in_the_code_object(so):
    """four instantiations (FAST x E) of each taps kernel, with the production kernels' LDS and launch bounds; the
    production kernels keep their eight each"""
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

    for kernel in ("ita_long_proj_taps_kernel", "ita_long_attn_taps_kernel"):
        got = named(kernel)
        assert len(got) == 4, f"{kernel}: {[n for n, _ in got]}"
        assert {re.search(r"ILb([01])ELi(\d+)E", n).groups() for n, _ in got} == {("0", "64"), ("1", "64"), ("0", "128"), ("1", "128")}
        for name, b in got:
            assert int(re.search(r"\.max_flat_workgroup_size:\s+(\d+)", b).group(1)) == 512, name
            assert int(re.search(r"\.vgpr_count:\s+(\d+)", b).group(1)) <= (128 if "attn" in kernel else 256), name
    for kernel in ("ita_long_proj_kernel", "ita_long_attn_kernel"):
        assert len(named(kernel)) == 8, kernel
