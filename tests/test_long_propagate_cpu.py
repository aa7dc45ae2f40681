"""CPU-side checks of the long-sequence propagation (ita_mha_long_int8_propagate, Engine.attention_propagate_long /
attention_rollout_long / attention_rollout_map_long): the numpy definition attention_propagate_ref against products taken
directly with mha_heads_ref.mha's probabilities, its closed form on the crafted frames of long_taps_common, the digit
planes of the rollout, the one-layer rollout of attention_rollout_ref, and the ABI: prototype, export, binding, signatures,
and the instantiations of ita_long_prop_kernel in the code object beside the unchanged counts of the five existing long
kernels.  No compute call is made here."""
import ctypes
import inspect
import os
import re
import shutil
import tempfile

import numpy as np
import pytest

from conftest import REPO
from drone_oa_iree_vit_accelerator_amd import attention_propagate_ref as apr
from drone_oa_iree_vit_accelerator_amd import attention_rollout_ref as arr
from drone_oa_iree_vit_accelerator_amd import attention_stats_ref as asr
from drone_oa_iree_vit_accelerator_amd import host
from drone_oa_iree_vit_accelerator_amd import mha_heads_ref as ref
from long_cases import long_case
import long_propagate_common as lpc
import long_taps_common as ltc

LLVM = "/opt/rocm/lib/llvm/bin"


@pytest.mark.parametrize("name", lpc.FIXTURES)
def test_propagate_is_the_product_with_the_definitions_probabilities(name):
    S, B = 256, 2
    _, t, _ = lpc.blob_case(name)
    x, w = lpc.frames(name, S, B), lpc.weights(S, B)
    p = ref.mha(x, t, 1, 0)[1]["probs"].astype(np.int64)
    want = w.astype(np.int64) @ p
    for block in (512, 96):          # one block, and blocks that do not divide S
        got = apr.propagate(x, t, w, 0, block=block)
        assert got.dtype == np.int32 and got.shape == (B, 64, S)
        np.testing.assert_array_equal(got, want)
    # the same weights for every frame
    np.testing.assert_array_equal(apr.propagate(x, t, w[0]), w[0].astype(np.int64) @ p)
    # all ones: attention received; one-hot: that probability row
    ones = np.ones((B, 1, S), np.int8)
    np.testing.assert_array_equal(apr.propagate(x, t, ones)[:, 0], asr.stats(x, t)["col_mass"])
    for r in (0, 127, 128, S - 1):
        np.testing.assert_array_equal(apr.propagate(x, t, lpc.one_hot(S, r)[None])[:, 0], p[:, r])
    assert np.abs(want).max() > 255


@pytest.mark.parametrize("form", lpc.CRAFTED)
def test_closed_form_on_crafted_frames(form):
    """every query of a frame shares the probability row y: out[r, j] = y[j] * sum_i w[r, i].  Rows of sum 32 768 and
    around 65 280, where the inverse's high byte runs out (the 256-key rows of the fixture have 65 280, 65 281 and 65 282;
    65 279 occurs among its 8192-key rows only), and a row the integer softmax kills"""
    d = ltc.fixture()
    sums = ltc.row_sums(d["x256"])
    pick = [int(np.flatnonzero(sums == s)[0]) for s in (32768, 32769, 65280, 65281, 65282)]
    pick.append(int(np.flatnonzero(d["y256"].astype(np.int64).sum(-1) == 0)[0]))
    _, t, _ = ltc.crafted(form)
    x = ltc.frames_for(form, d["x256"][pick])
    w = lpc.weights(256, len(pick))
    got = apr.propagate(x, t, w)
    for b in range(len(pick)):
        want = w[b].astype(np.int64).sum(-1)[:, None] * d["y256"][pick[b]].astype(np.int64)[None]
        np.testing.assert_array_equal(got[b], want, err_msg=f"{form} fixture row {pick[b]}")


def test_digit_planes_reproduce_the_wide_product():
    rs = np.random.RandomState(5)
    S, n = 256, 7
    q = rs.randint(0, 1 << 21, size=(2, n, S)).astype(np.int64)
    q[0, 0, :4] = (0, (1 << 21) - 1, 127, 128)
    q[1, n - 1] = (1 << 21) - 1
    p = rs.randint(0, 256, size=(2, S, S)).astype(np.int64)
    d = host.rollout_digits(q)
    assert d.dtype == np.int8 and d.shape == (2, 3 * n, S) and d.min() == 0 and d.max() == 127
    for k in range(3):
        np.testing.assert_array_equal(d[:, k * n:(k + 1) * n], (q >> (7 * k)) & 127)
    prod = d.astype(np.int64) @ p
    assert np.abs(prod).max() < 2 ** 31             # what the primitive returns as int32
    got = host.rollout_combine(prod.astype(np.int32))
    assert got.dtype == np.int64
    np.testing.assert_array_equal(got, q @ p)
    for bad in (-1, 1 << 21):
        with pytest.raises(ValueError):
            host.rollout_digits(np.array([[bad]]))
    assert host.ROLLOUT_QMAX == arr.QMAX == (1 << 21) - 1 and host.ROLLOUT_CHUNK == 21


def test_one_layer_rollout_of_a_one_hot(oracle):
    name = "vitlstm_E64_seed0_B2"
    case = long_case(name)
    nl, t, fp = case.num_layers, case.t, case.fp
    assert nl == 1
    S, B, rows = 256, 2, (0, 100, 255)
    x = lpc.frames(name, S, B)
    p = ref.mha(x, t, 1, 0)[1]["probs"]
    got = arr.rollout(oracle, x, t, fp, nl, rows)
    assert got.dtype == np.float64 and got.shape == (B, 3, S)
    for n, r in enumerate(rows):
        e = np.zeros(S)
        e[r] = 1.0
        np.testing.assert_array_equal(got[:, n], 0.5 * (e + p[:, r].astype(np.float64) / 256.0))
    # the uniform start: 0.5 (1 / S + mean of the rows / 256) to rounding, and exactly the written-down recurrence
    u = arr.rollout(oracle, x, t, fp, nl, None)
    assert u.shape == (B, 1, S)
    q = np.full((B, 1, S), arr.QMAX, np.int64)
    want = 0.5 * (1.0 / S + ((q @ p.astype(np.int64)).astype(np.float64) * ((1.0 / S) / arr.QMAX)) / 256.0)
    np.testing.assert_array_equal(u, want)


@pytest.fixture(scope="module")
def so():
    return host.build_extension()


def _header():
    hdr = open(os.path.join(REPO, "include", "ita_mi355x.h")).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_symbol_declared_listed_and_exported(so):
    assert re.search(r"\bint\s+ita_mha_long_int8_propagate\s*\(\s*ita_handle\s+h\s*,\s*int\s+layer\s*,\s*const\s+float\s*\*\s*x_dev\s*,"
                     r"\s*int\s+batch\s*,\s*int\s+seq_len\s*,\s*const\s+int8_t\s*\*\s*w_dev\s*,\s*int\s+n_w\s*,"
                     r"\s*int32_t\s*\*\s*out_dev\s*,\s*void\s*\*\s*stream\s*\)", _header())
    assert "ita_mha_long_int8_propagate" in host.EXPORTED_SYMBOLS
    lib = ctypes.CDLL(so)
    assert hasattr(lib, "ita_mha_long_int8_propagate")
    assert lib.ita_abi_version() == 1
    vp, i = ctypes.c_void_p, ctypes.c_int
    assert host.lib().ita_mha_long_int8_propagate.argtypes == [vp, i, vp, i, i, vp, i, vp, vp]
    assert host.LONG_MAX_WEIGHT_ROWS == 64


def test_python_signatures():
    sig = inspect.signature(host.Engine.attention_propagate_long)
    assert list(sig.parameters) == ["self", "x", "w", "layer"] and sig.parameters["layer"].default == 0
    sig = inspect.signature(host.Engine.attention_rollout_long)
    assert list(sig.parameters) == ["self", "x", "rows", "first_layer"]
    assert sig.parameters["rows"].default is None and sig.parameters["first_layer"].default == 0
    sig = inspect.signature(host.Engine.attention_rollout_map_long)
    assert list(sig.parameters) == ["self", "frames", "tok_h", "tok_w", "queries", "depth_scale"]
    assert sig.parameters["queries"].default is None and sig.parameters["depth_scale"].default is None


def test_kernels_in_the_code_object(so):
    """ita_long_prop_kernel: two instantiations (FAST or not: E does not appear), 512 threads, at most 128 registers, no
    scratch; the five existing long kernels keep their instantiation counts"""
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
        pat = rf"\.name:\s+(_Z\d+{kernel}I\S+)"
        return [(re.search(pat, b).group(1), b) for b in blocks if re.search(pat, b)]

    got = named("ita_long_prop_kernel")
    assert len(got) == 2, [n for n, _ in got]
    assert {re.search(r"ILb([01])E", n).group(1) for n, _ in got} == {"0", "1"}
    for name, b in got:
        assert int(re.search(r"\.max_flat_workgroup_size:\s+(\d+)", b).group(1)) == 512, name
        assert int(re.search(r"\.vgpr_count:\s+(\d+)", b).group(1)) <= 128, name          # four waves per SIMD
        assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", b).group(1)) == 0, name
    assert any(re.search(r"\.name:\s+_Z\d+ita_long_prop_prep_kernel", b) for b in blocks)
    for kernel, count in (("ita_long_proj_kernel", 8), ("ita_long_attn_kernel", 8), ("ita_long_proj_taps_kernel", 4),
                          ("ita_long_attn_taps_kernel", 4), ("ita_long_stats_kernel", 2)):
        assert len(named(kernel)) == count, (kernel, [n for n, _ in named(kernel)])
