"""CPU-side checks of the long-sequence layer (ita_mha_long_int8 / ita_encoder_layer_long, Engine.mha_long /
encoder_layer_long / encode_long): the symbols are declared, listed and exported, the Python signatures are in place, and
no instantiation of the two long kernels uses more scratch per lane than the largest one had before they were templated
on E and the I/O form ("Long-sequence layer": the code-object table).  No compute call is made here."""
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
SYMBOLS = ("ita_mha_long_int8", "ita_encoder_layer_long")
# .private_segment_fixed_size of ita_long_attn_kernel<FAST = true> (E = 128, int8 I/O) at the commit before this layer
# existed, the largest of the then four long kernels; a recorded figure, not read from this build
PARENT_MAX_SCRATCH_BYTES = 52
# FAST x E x I/O form, for each of the two kernels
INSTANTIATIONS = 2 * 2 * 2


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
    sig = inspect.signature(host.Engine.mha_long)
    assert list(sig.parameters) == ["self", "x", "layer"] and sig.parameters["layer"].default == 0
    sig = inspect.signature(host.Engine.encoder_layer_long)
    assert list(sig.parameters) == ["self", "x", "layer", "out"]
    assert sig.parameters["layer"].default == 0 and sig.parameters["out"].default is None
    assert list(inspect.signature(host.Engine.encode_long).parameters) == ["self", "x"]


def test_long_kernels_scratch_within_the_recorded_bound(so):
    """the extracted gfx950 code object's metadata: every ita_long_proj_kernel / ita_long_attn_kernel instantiation is
    there, and none has a larger .private_segment_fixed_size than the recorded figure"""
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
    for kernel in ("ita_long_proj_kernel", "ita_long_attn_kernel"):
        pat = r"\.name:\s+(_Z\d+%sI\S+)" % kernel
        blocks = [(re.search(pat, b).group(1), b) for b in notes.split("- .agpr_count:")[1:] if re.search(pat, b)]
        assert len(blocks) == INSTANTIATIONS, f"{kernel}: {[n for n, _ in blocks]}"
        for name, b in blocks:
            m = re.search(r"\.private_segment_fixed_size:\s+(\d+)", b)
            assert m, f"no .private_segment_fixed_size in the metadata of {name}"
            assert int(m.group(1)) <= PARENT_MAX_SCRATCH_BYTES, f"{name} uses {m.group(1)} bytes of scratch per lane"
