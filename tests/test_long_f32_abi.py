"""CPU-side checks of the long float attention (ita_mha_long_f32 / ita_encoder_layer_long_f32, Engine.mha_long_f32 /
encoder_layer_long_f32 / encode_long_f32 / encode_frames_long_f32): the symbols are declared, listed and exported, the
Python signatures are in place, and the gfx950 code object holds both E instantiations of ita_lf32_proj_kernel and
ita_lf32_attn_kernel, none with scratch ("Long float attention": the code-object table).  Register,
scratch and LDS metadata only; no compute call is made here."""
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
SYMBOLS = ("ita_mha_long_f32", "ita_encoder_layer_long_f32")
LDS_PER_CU = 160 * 1024


@pytest.fixture(scope="module")
def so():
    return host.build_extension()


def test_symbols_declared_listed_and_exported(so):
    hdr = open(os.path.join(REPO, "include", "ita_mi355x.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = ctypes.CDLL(so)
    for name in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(\s*ita_handle\s+h\s*,\s*int\s+layer\s*,\s*const\s+float\s*\*\s*x_dev\s*,\s*float\s*\*\s*y_dev\s*,"
                         r"\s*int\s+batch\s*,\s*int\s+seq_len\s*,\s*void\s*\*\s*stream\s*\)" % name, hdr), name
        assert name in host.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
    assert lib.ita_abi_version() == 1


def test_python_signatures():
    sig = inspect.signature(host.Engine.mha_long_f32)
    assert list(sig.parameters) == ["self", "x", "layer"] and sig.parameters["layer"].default == 0
    sig = inspect.signature(host.Engine.encoder_layer_long_f32)
    assert list(sig.parameters) == ["self", "x", "layer", "out"]
    assert sig.parameters["layer"].default == 0 and sig.parameters["out"].default is None
    assert list(inspect.signature(host.Engine.encode_long_f32).parameters) == ["self", "x"]
    sig = inspect.signature(host.Engine.encode_frames_long_f32)
    assert list(sig.parameters) == ["self", "frames", "tok_h", "tok_w", "depth_scale"]
    assert sig.parameters["depth_scale"].default is None


def test_long_f32_kernels_present_without_scratch(so):
    """the extracted gfx950 code object's metadata: ita_lf32_proj_kernel<64 | 128> and ita_lf32_attn_kernel<64 | 128> are
    there, none has scratch or spills, and their static LDS leaves room for the attention kernel's dynamic 144 KB"""
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
    for kernel in ("ita_lf32_proj_kernel", "ita_lf32_attn_kernel"):
        pat = r"\.name:\s+(_Z\d+%sILi(\d+)E\S+)" % kernel
        blocks = {int(re.search(pat, b).group(2)): b for b in notes.split("- .agpr_count:")[1:] if re.search(pat, b)}
        assert sorted(blocks) == [64, 128], f"{kernel}: instantiations {sorted(blocks)}"
        for E, b in blocks.items():
            field = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, b).group(1))
            assert field("private_segment_fixed_size") == 0, f"{kernel}<{E}> uses scratch"
            assert field("vgpr_spill_count") == 0 and field("sgpr_spill_count") == 0, f"{kernel}<{E}> spills"
            assert field("vgpr_count") <= 256, f"{kernel}<{E}>: below two waves per SIMD"
            assert field("group_segment_fixed_size") + 3 * 49152 <= LDS_PER_CU
