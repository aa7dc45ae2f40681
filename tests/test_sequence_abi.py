"""CPU-side checks of the sequence capability (ita_vitlstm_sequence / Engine.forward_sequence / replay's schedule): the
symbol is declared, listed and exported, the Python signatures are in place, and the time-loop kernel's code object uses
no scratch memory.  No compute call is made here."""
import ctypes
import inspect
import os
import re
import shutil
import tempfile

import pytest

from conftest import REPO
from drone_oa_iree_vit_accelerator_amd import host, replay

LLVM = "/opt/rocm/lib/llvm/bin"


@pytest.fixture(scope="module")
def so():
    return host.build_extension()


def test_symbol_declared_listed_and_exported(so):
    hdr = open(os.path.join(REPO, "include", "ita_mi355x.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+ita_vitlstm_sequence\s*\(", hdr)
    assert "ita_vitlstm_sequence" in host.EXPORTED_SYMBOLS
    lib = ctypes.CDLL(so)
    assert hasattr(lib, "ita_vitlstm_sequence")
    assert lib.ita_abi_version() == 1


def test_python_signatures():
    sig = inspect.signature(host.Engine.forward_sequence)
    assert list(sig.parameters) == ["self", "imgs", "desvels", "quats", "hidden", "lengths", "out"]
    assert all(sig.parameters[k].default is None for k in ("quats", "hidden", "lengths", "out"))
    rs = inspect.signature(replay.replay)
    assert list(rs.parameters) == ["engine", "root", "max_batch", "schedule"]
    assert rs.parameters["schedule"].default == "steps" and rs.parameters["max_batch"].default == 1024


def test_replay_rejects_unknown_schedule_before_touching_the_engine(tmp_path):
    class NoEngine:
        def __getattr__(self, name):
            raise AssertionError(f"the engine was touched ({name}) before the schedule was checked")
    with pytest.raises(ValueError):
        replay.replay(NoEngine(), str(tmp_path / "missing"), schedule="frames")


def test_seq_kernel_uses_no_scratch(so):
    """the extracted gfx950 code object's metadata for ita_lstm_seq_kernel: .private_segment_fixed_size 0"""
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
    blocks = [b for b in notes.split("- .agpr_count:")[1:] if re.search(r"\.name:\s+_Z\d+ita_lstm_seq_kernel", b)]
    if not blocks:      # metadata layout not split as expected: find the kernel's entry by its name line
        blocks = [notes[m.start() - 2000:m.start() + 2000] for m in re.finditer(r"\.name:\s+_Z\d+ita_lstm_seq_kernel", notes)]
    assert blocks, "ita_lstm_seq_kernel is not in the code object's metadata"
    for b in blocks:
        m = re.search(r"\.private_segment_fixed_size:\s+(\d+)", b)
        assert m, "no .private_segment_fixed_size in the kernel's metadata"
        assert int(m.group(1)) == 0, f"ita_lstm_seq_kernel uses {m.group(1)} bytes of scratch per lane"
