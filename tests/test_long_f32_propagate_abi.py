"""CPU-side ABI checks of the long float propagation (ita_mha_long_f32_propagate, Engine.attention_propagate_long_f32 /
attention_rollout_long_f32 / attention_rollout_map_long_f32): the prototype is in the header, the symbol is listed and
exported, the Python signatures are in place beside their unchanged int8 siblings, the new kernels are in the gfx950 code
object (ita_lf32_projkq_kernel for E = 64 and 128, ita_lf32_prop_kernel once: it does not depend on E) with 512 threads, at
most 256 registers, no spill and no scratch, and the production ita_lf32_* kernels keep their instantiation counts.  No
compute call is made here."""
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


def test_symbol_declared_listed_and_exported(so):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "ita_mi355x.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+ita_mha_long_f32_propagate\s*\(\s*ita_handle\s+h\s*,\s*int\s+layer\s*,\s*const\s+float\s*\*\s*x_dev\s*,"
                     r"\s*int\s+batch\s*,\s*int\s+seq_len\s*,\s*const\s+float\s*\*\s*w_dev\s*,\s*int\s+n_w\s*,\s*float\s*\*\s*out_dev\s*,"
                     r"\s*void\s*\*\s*stream\s*\)", hdr)
    assert "ita_mha_long_f32_propagate" in host.EXPORTED_SYMBOLS
    lib = ctypes.CDLL(so)
    assert hasattr(lib, "ita_mha_long_f32_propagate")
    assert lib.ita_abi_version() == 1
    assert host.lib().ita_mha_long_f32_propagate.argtypes == host.lib().ita_mha_long_int8_propagate.argtypes
    # the refusal of an int8 layer names the sibling; the int8 sibling keeps its own words
    src = open(os.path.join(REPO, "drone-oa-iree-vit-accelerator_amd", "csrc", "ita_plugin.hip")).read()
    assert "ita_mha_long_int8_propagate propagates through it" in src
    assert "ita_mha_long_int8_propagate: n_w must be in [1, 64]" in src


def test_python_signatures():
    E = host.Engine
    sig = inspect.signature(E.attention_propagate_long_f32)
    assert list(sig.parameters) == ["self", "x", "w", "layer"] and sig.parameters["layer"].default == 0
    sig = inspect.signature(E.attention_rollout_long_f32)
    assert list(sig.parameters) == ["self", "x", "rows", "first_layer"]
    assert sig.parameters["rows"].default is None and sig.parameters["first_layer"].default == 0
    sig = inspect.signature(E.attention_rollout_map_long_f32)
    assert list(sig.parameters) == ["self", "frames", "tok_h", "tok_w", "queries", "depth_scale"]
    assert sig.parameters["queries"].default is None and sig.parameters["depth_scale"].default is None
    # the int8 siblings keep theirs
    for f32, int8 in ((E.attention_propagate_long_f32, E.attention_propagate_long), (E.attention_rollout_long_f32, E.attention_rollout_long),
                      (E.attention_rollout_map_long_f32, E.attention_rollout_map_long)):
        assert str(inspect.signature(f32)) == str(inspect.signature(int8))
    assert host.ROLLOUT_F32_CHUNK == host.LONG_MAX_WEIGHT_ROWS == 64 and host.ROLLOUT_CHUNK == 21


def test_kernels_in_the_code_object(so):
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

    def named(kernel, templated=True):
        pat = r"\.name:\s+(_Z\d+%s%s\S*)" % (kernel, "I" if templated else r"\d")
        return [(re.search(pat, b).group(1), b) for b in blocks if re.search(pat, b)]

    def field(b, name):
        return int(re.search(r"\.%s:\s+(\d+)" % name, b).group(1))

    proj, prop = named("ita_lf32_projkq_kernel"), named("ita_lf32_prop_kernel", templated=False)
    assert len(proj) == 2 and {re.search(r"ILi(\d+)E", n).group(1) for n, _ in proj} == {"64", "128"}, [n for n, _ in proj]
    assert len(prop) == 1, [n for n, _ in prop]
    for name, b in proj + prop:
        assert field(b, "max_flat_workgroup_size") == 512, name
        assert field(b, "vgpr_count") + int(b.split()[0]) <= 256 and field(b, "private_segment_fixed_size") == 0, name
        assert field(b, "vgpr_spill_count") == 0 and field(b, "sgpr_spill_count") == 0, name
    # the production kernels and the siblings keep their instantiation counts
    for kernel in ("ita_lf32_proj_kernel", "ita_lf32_attn_kernel", "ita_lf32_proj_taps_kernel", "ita_lf32_attn_taps_kernel",
                   "ita_lf32_stats_kernel"):
        assert len(named(kernel)) == 2, kernel
    all_lf32 = [b for b in blocks if re.search(r"\.name:\s+_Z\d+ita_lf32_", b)]
    assert len(all_lf32) == 10 + 2 + 3, "ita_lf32_probs_kernel, ita_lf32_colsum_kernel and the three new ones beside the ten"
