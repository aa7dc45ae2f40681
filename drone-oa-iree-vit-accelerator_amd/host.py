"""Host side of the MI355X ITA engine: ctypes binding of ``csrc/libita_mi355x.so`` (C ABI in
include/ita_mi355x.h) and a mirror of the reference's model interface.

PyTorch is used for device memory, streams and (in bench.py) torch.distributed only; all
arithmetic happens in the HIP kernels behind the C ABI.  There is deliberately NO CPU or
eager fallback: if the extension is missing or no GPU is visible, calls raise.

Reference interface mirrored here (all paths relative to the reference repository):
  ITALSTMNetVIT_QAT.forward(X)   models/ITA_single_layer_upsample_shuffle/QAT/model.py:93-132
      X = [img (B,1,60,90), desvel (B,1), quat (B,4) | None, (h, c) | None] -> (vel (B,3), (h, c))
  refine_inputs                  same file :22-31 (default quaternion, resize to 60x90)
  ITASelfAttention_QAT / ITAFeedForward_QAT   models/ITA/QAT/layers.py:47-127
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from typing import Optional, Sequence

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "csrc")
_SO = os.path.join(_CSRC, "libita_mi355x.so")
_REPO = os.path.dirname(_HERE)
_LIB = None

IMAGE_F32, IMAGE_U8 = 0, 1
PIXEL_U8, PIXEL_U16, PIXEL_F32 = 0, 1, 2
INGEST_MAX_DIM = 4096          # ita_ingest: height and width in [1, 4096]
DISPATCH_F16, DISPATCH_F32 = 0, 1
FFN_INT8, FFN_F32 = 0, 1
ATTN_INT8, ATTN_F32 = 0, 1
HEAD_TIMEOUT = 1

EXPORTED_SYMBOLS = (
    "ita_abi_version", "ita_create", "ita_destroy", "ita_load_weights", "ita_validate_blob", "ita_reserve", "ita_get_dims",
    "ita_last_error", "ita_error_string", "ita_mha_int8", "ita_mha_int8_taps", "ita_mha_q8", "ita_mha_long_q8", "ita_mha_long_int8", "ita_mha_long_int8_taps", "ita_mha_long_int8_stats", "ita_mha_long_int8_hist", "ita_mha_long_int8_propagate", "ita_encoder_layer_long", "ita_ffn_int8", "ita_ffn_int8_taps",
    "ita_ffn_f32", "ita_get_ffn_kind", "ita_mha_f32", "ita_get_attn_kind", "ita_mha_long_f32", "ita_mha_long_f32_taps", "ita_mha_long_f32_stats", "ita_mha_long_f32_propagate", "ita_encoder_layer_long_f32",
    "ita_encoder_layer", "ita_tokenizer", "ita_fusion_tail", "ita_vitlstm_forward", "ita_bind_dispatch",
    "ita_profile_begin", "ita_profile_begin_sampled", "ita_profile_end", "ita_set_tail_mode", "ita_debug_encoder_stamps",
    "ita_fusion_tail_load", "ita_fusion_tail_large",
    "ita_wire_unpack_packet", "ita_wire_postprocess", "ita_vitlstm_forward_slots", "ita_vitlstm_front",
    "ita_vitlstm_back", "ita_vitlstm_pipelined", "ita_vitlstm_front_ev", "ita_vitlstm_encode", "ita_vitlstm_fold", "ita_vitlstm_tail", "ita_debug_softmax_rows",
    "ita_head_status", "ita_vitlstm_sequence", "ita_ingest", "ita_tokenizer_long", "ita_ingest_wire", "ita_ingest_wire_prepare", "ita_resize_table",
    "ita_debug_fast_site_ok", "ita_debug_layer_forms", "ita_debug_fused_site", "ita_debug_fused_check", "ita_debug_layer_fused",
    "ita_debug_dequant_site", "ita_debug_layer_dequant", "ita_debug_x2_planes",
    "ITASelfAttention_workgroup", "ITASelfAttention_workgroup_expanded", "ITAFeedForward_workgroup",
)

HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
               "-Wall", "-Wno-unused-function"]


class ITAError(RuntimeError):
    pass


def build_extension(force: bool = False, verbose: bool = False) -> str:
    """hipcc cross-compiles the plugin for gfx950 in-tree (works without a GPU)."""
    srcs = [os.path.join(_CSRC, f) for f in os.listdir(_CSRC) if f.endswith((".hip", ".h"))]
    srcs += [os.path.join(_REPO, "include", f) for f in ("ita_mi355x.h", "ita_weights.h")]
    if not force and os.path.exists(_SO) and all(os.path.getmtime(_SO) >= os.path.getmtime(s) for s in srcs):
        return _SO
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc] + HIPCC_FLAGS + ["-I", os.path.join(_REPO, "include"), os.path.join(_CSRC, "ita_plugin.hip"),
                                   "-o", _SO]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return _SO


def build_samples(force: bool = False, verbose: bool = False) -> str:
    """the UDP inference host (reference samples/inference_udp_FPGA_custom_dispatch/main.cpp)"""
    src = os.path.join(_HERE, "samples", "ita_udp_server.cpp")
    exe = os.path.join(_HERE, "samples", "ita_udp_server")
    deps = [src, _SO, os.path.join(_REPO, "include", "ita_wire.h"), os.path.join(_REPO, "include", "ita_mi355x.h")]
    if not force and os.path.exists(exe) and all(os.path.getmtime(exe) >= os.path.getmtime(d) for d in deps):
        return exe
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "-O2", "-std=c++17", "-Wall", "-I", os.path.join(_REPO, "include"), src, "-L", _CSRC,
           "-lita_mi355x", "-Wl,-rpath,$ORIGIN/../csrc", "-o", exe]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return exe


class _MhaTaps(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("x_q", "Q", "K", "V", "logits", "probs", "ctx", "out_q")]


class _MhaLongTaps(C.Structure):      # ita_mha_long_taps
    _fields_ = [(n, C.c_void_p) for n in ("x_q", "Q", "K", "V", "ctx", "out_q")] + \
               [("rows", C.POINTER(C.c_int)), ("n_rows", C.c_int)] + \
               [(n, C.c_void_p) for n in ("logits", "probs", "row_max", "row_sum")]


LONG_TENSOR_TAPS = ("x_q", "Q", "K", "V", "ctx", "out_q")
LONG_ROW_TAPS = ("logits", "probs", "row_max", "row_sum")
LONG_MAX_ROWS = 1024


class _MhaLongStats(C.Structure):     # ita_mha_long_stats
    _fields_ = [(n, C.c_void_p) for n in ("row_max", "row_sum", "row_mass", "row_nnz", "col_mass", "col_nnz")]


LONG_STATS = ("row_max", "row_sum", "row_mass", "row_nnz", "col_mass", "col_nnz")


class _MhaLongHist(C.Structure):      # ita_mha_long_hist
    _fields_ = [(n, C.c_void_p) for n in ("logits", "shifts", "probs", "logits_out", "acc_range")]


LONG_HIST = ("logits", "logits_out", "acc_range", "shifts", "probs")      # the order of attention_hist_ref.NAMES
LONG_HIST_STAGES = ("x_q", "Q", "K", "V", "ctx", "out_q")
LONG_MAX_WEIGHT_ROWS = 64      # ita_mha_long_int8_propagate: n_w in [1, 64]
ROLLOUT_QMAX = 2097151         # attention rollout: a vector is quantised to 21 bits, three base-128 digits
ROLLOUT_CHUNK = LONG_MAX_WEIGHT_ROWS // 3      # vectors per ita_mha_long_int8_propagate call
ROLLOUT_F32_CHUNK = LONG_MAX_WEIGHT_ROWS       # vectors per ita_mha_long_f32_propagate call


def rollout_digits(q):
    """the three base-128 digit planes of q: integers in [0, 2^21), (..., n, S) -> int8 (..., 3 n, S) with row k n + j =
    (q[j] >> 7 k) & 127 (numpy)"""
    import numpy as np
    q = np.asarray(q, np.int64)
    if q.min(initial=0) < 0 or q.max(initial=0) > ROLLOUT_QMAX:
        raise ValueError("rollout_digits takes integers in [0, 2^21)")
    return np.concatenate([(q >> (7 * k)) & 127 for k in range(3)], axis=-2).astype(np.int8)


def rollout_combine(d):
    """d = rollout_digits(q) @ P, integer (..., 3 n, S) -> q @ P = sum_k 128^k d[k n : (k + 1) n], int64 (..., n, S) (numpy)"""
    import numpy as np
    d = np.asarray(d).astype(np.int64)
    n = d.shape[-2] // 3
    assert d.shape[-2] == 3 * n, d.shape
    return d[..., :n, :] + (d[..., n:2 * n, :] << 7) + (d[..., 2 * n:, :] << 14)


class _MhaLongF32Taps(C.Structure):   # ita_mha_long_f32_taps
    _fields_ = [(n, C.c_void_p) for n in ("Q", "K", "V", "ctx")] + \
               [("rows", C.POINTER(C.c_int)), ("n_rows", C.c_int)] + \
               [(n, C.c_void_p) for n in ("logits", "probs", "row_max", "row_sum")]


LONG_F32_TENSOR_TAPS = ("Q", "K", "V", "ctx")


class _MhaLongF32Stats(C.Structure):  # struct ita_mha_long_f32_stats
    _fields_ = [(n, C.c_void_p) for n in ("row_max", "row_sum", "row_gap", "row_nnz", "col_mass", "col_nnz")]


LONG_F32_STATS = ("row_max", "row_sum", "row_gap", "row_nnz", "col_mass", "col_nnz")


class _FfnTaps(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("x_q", "h", "out_q")]


class _FwdTaps(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("tokens", "x1", "x2", "feat", "dec")]


def lib():
    """Loads the C-ABI library; fails loudly when it has not been built."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(_SO):
            raise ITAError(f"{_SO} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(there is no CPU fallback)")
        L = C.CDLL(_SO)
        L.ita_error_string.restype = C.c_char_p
        vp, i = C.c_void_p, C.c_int
        L.ita_create.argtypes = [C.POINTER(vp), i]
        L.ita_destroy.argtypes = [vp]
        L.ita_load_weights.argtypes = [vp, vp, C.c_size_t]
        L.ita_reserve.argtypes = [vp, i]
        L.ita_get_dims.argtypes = [vp] + [C.POINTER(i)] * 6
        L.ita_mha_int8.argtypes = [vp, i, vp, vp, i, vp]
        L.ita_mha_int8_taps.argtypes = [vp, i, vp, vp, i, C.POINTER(_MhaTaps), vp]
        L.ita_ffn_int8.argtypes = [vp, i, vp, vp, i, vp]
        L.ita_ffn_int8_taps.argtypes = [vp, i, vp, vp, i, C.POINTER(_FfnTaps), vp]
        L.ita_ffn_f32.argtypes = [vp, i, vp, vp, i, vp]
        L.ita_get_ffn_kind.argtypes = [vp, i, C.POINTER(i)]
        L.ita_mha_f32.argtypes = [vp, i, vp, vp, i, vp]
        L.ita_get_attn_kind.argtypes = [vp, i, C.POINTER(i)]
        L.ita_head_status.argtypes = [vp, C.POINTER(i)]
        L.ita_encoder_layer.argtypes = [vp, i, vp, vp, i, vp]
        L.ita_tokenizer.argtypes = [vp, vp, i, vp, i, vp]
        L.ita_fusion_tail.argtypes = [vp, vp, vp, i, vp]
        L.ita_vitlstm_forward.argtypes = [vp, vp, i, vp, vp, vp, vp, vp, vp, vp, i, C.POINTER(_FwdTaps), vp]
        L.ita_vitlstm_forward_slots.argtypes = [vp, vp, i, vp, vp, vp, vp, vp, i, vp, i, vp]
        L.ita_vitlstm_front.argtypes = [vp, vp, i, i, i, vp]
        L.ita_vitlstm_front_ev.argtypes = [vp, vp, i, i, i, vp, vp]
        L.ita_vitlstm_encode.argtypes = [vp, vp, i, i, i, vp]
        L.ita_vitlstm_fold.argtypes = [vp, i, i, i, vp]
        L.ita_vitlstm_back.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, i, i, vp]
        L.ita_vitlstm_pipelined.argtypes = [vp, vp, i, vp, vp, vp, vp, vp, i, i, vp, vp]
        L.ita_vitlstm_sequence.argtypes = [vp, vp, i, vp, vp, vp, vp, vp, vp, i, i, vp]
        L.ita_ingest.argtypes = [vp, vp, i, i, i, C.c_longlong, C.c_longlong, C.c_float, vp, i, vp]
        L.ita_tokenizer_long.argtypes = [vp, vp, i, i, i, C.c_longlong, C.c_longlong, C.c_float, i, i, vp, i, vp]
        L.ita_ingest_wire.argtypes = [vp, vp, i, i, C.c_longlong, C.c_longlong, vp, i, vp]
        L.ita_ingest_wire_prepare.argtypes = [vp, i, i]
        L.ita_resize_table.argtypes = [i, i, vp, vp, vp, i, C.POINTER(i)]
        L.ita_mha_q8.argtypes = [vp, i, vp, vp, i, vp]
        L.ita_mha_long_q8.argtypes = [vp, i, vp, vp, i, i, vp]
        L.ita_mha_long_int8.argtypes = [vp, i, vp, vp, i, i, vp]
        L.ita_mha_long_int8_taps.argtypes = [vp, i, vp, vp, i, i, C.POINTER(_MhaLongTaps), vp]
        L.ita_mha_long_int8_stats.argtypes = [vp, i, vp, i, i, C.POINTER(_MhaLongStats), vp]
        L.ita_mha_long_int8_hist.argtypes = [vp, i, vp, i, i, C.POINTER(_MhaLongHist), vp]
        L.ita_mha_long_int8_propagate.argtypes = [vp, i, vp, i, i, vp, i, vp, vp]
        L.ita_encoder_layer_long.argtypes = [vp, i, vp, vp, i, i, vp]
        L.ita_mha_long_f32.argtypes = [vp, i, vp, vp, i, i, vp]
        L.ita_mha_long_f32_taps.argtypes = [vp, i, vp, vp, i, i, C.POINTER(_MhaLongF32Taps), vp]
        L.ita_mha_long_f32_stats.argtypes = [vp, i, vp, i, i, C.c_float, C.POINTER(_MhaLongF32Stats), vp]
        L.ita_mha_long_f32_propagate.argtypes = [vp, i, vp, i, i, vp, i, vp, vp]
        L.ita_encoder_layer_long_f32.argtypes = [vp, i, vp, vp, i, i, vp]
        L.ita_vitlstm_tail.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, i, vp]
        L.ita_debug_softmax_rows.argtypes = [vp, vp, vp, i, vp]
        L.ita_debug_fast_site_ok.argtypes = [C.c_float]
        L.ita_debug_layer_forms.argtypes = [vp, i, C.POINTER(C.c_uint), C.POINTER(i)]
        L.ita_debug_fused_site.argtypes = [C.c_float, C.POINTER(i), C.POINTER(C.c_float)]
        L.ita_debug_fused_check.argtypes = [C.c_float, i, i, C.POINTER(C.c_float)]
        L.ita_debug_layer_fused.argtypes = [vp, i, C.POINTER(C.c_uint), C.POINTER(i), C.POINTER(i), C.POINTER(C.c_float)]
        L.ita_debug_dequant_site.argtypes = [C.c_float, i, C.POINTER(i), C.POINTER(C.c_float)]
        L.ita_debug_layer_dequant.argtypes = [vp, i, C.POINTER(i), C.POINTER(i), C.POINTER(C.c_float)]
        L.ita_debug_x2_planes.argtypes = [vp, i, vp, vp, i, C.POINTER(i), vp]
        L.ita_validate_blob.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p]
        L.ita_bind_dispatch.argtypes = [vp, i, i]
        L.ita_wire_unpack_packet.argtypes = [vp, C.c_size_t, i, vp]
        L.ita_wire_postprocess.argtypes = [vp, C.c_float, C.c_float, vp]
        L.ita_wire_postprocess.restype = None
        L.ita_set_tail_mode.argtypes = [vp, i]
        L.ita_debug_encoder_stamps.argtypes = [vp, i, vp, vp, vp, i, vp, vp]
        L.ita_fusion_tail_load.argtypes = [vp, vp, vp, i, i]
        L.ita_fusion_tail_large.argtypes = [vp, vp, vp, i, i, i, vp]
        L.ita_profile_begin.argtypes = [vp, i]
        L.ita_profile_begin_sampled.argtypes = [vp, i, i, i]
        L.ita_profile_end.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(i)]
        L.ITASelfAttention_workgroup.argtypes = [vp, vp]
        L.ITASelfAttention_workgroup.restype = None
        L.ITAFeedForward_workgroup.argtypes = [vp, vp]
        L.ITAFeedForward_workgroup.restype = None
        L.ITASelfAttention_workgroup_expanded.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.c_size_t] * 2
        L.ITASelfAttention_workgroup_expanded.restype = None
        _LIB = L
    return _LIB


def _chk(rc: int):
    if rc != 0:
        raise ITAError(f"ita status {rc}: {lib().ita_error_string().decode()}")


def _torch():
    import torch
    return torch


def np_prod(shape) -> int:
    n = 1
    for d in shape:
        n *= int(d)
    return n


def _stream_ptr(device=None):
    """handle of torch's current stream ON `device` (an Engine passes its own ordinal: the current stream of whatever
    device happens to be current would belong to another GPU)"""
    return C.c_void_p(_torch().cuda.current_stream(device).cuda_stream)


def _dev_f32(t, shape=None):
    torch = _torch()
    if not t.is_cuda:
        raise ITAError("tensors handed to the ITA engine must live on the GPU (no CPU fallback)")
    t = t.contiguous()
    if t.dtype != torch.float32:
        t = t.float()
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ITAError(f"expected shape {tuple(shape)}, got {tuple(t.shape)}")
    return t


def resize_table(n_in: int, n_out: int):
    """ita_resize_table: one axis of the wire ingest's filter tables, built on the host (no GPU, no handle) ->
    (n0[n_out] int32, count[n_out] int32, coeff[n_out, width] float32), as ingest_wire_ref.resize_tables returns them"""
    import numpy as np
    cap = 4 * INGEST_MAX_DIM + 8                          # wider than any table of a source of at most 4096 pixels
    n0, count = np.zeros(n_out, np.int32), np.zeros(n_out, np.int32)
    coeff = np.zeros((max(n_out, 1), cap), np.float32)
    width = C.c_int(0)
    _chk(lib().ita_resize_table(n_in, n_out, n0.ctypes.data, count.ctypes.data, coeff.ctypes.data, cap, C.byref(width)))
    return n0, count, coeff[:, :width.value].copy()


FORMS_ATTN_IMAGE, FORMS_LAYER_IMAGE, FORMS_TOK_IMAGE = 1, 2, 4


def fast_site_ok(mult: float) -> bool:
    """ita_debug_fast_site_ok: the load-time proof that a requantisation site with this float32 multiplier may round once
    (host only: no GPU, no handle)"""
    return bool(lib().ita_debug_fast_site_ok(C.c_float(float(mult))))


ACC_BIAS = 0x4B400000      # the default accumulator base of the stream kernels: the pattern of the float 1.5 * 2^23
FUSED_SITES = ("Q", "K", "V", "L", "C")   # bit order of the fused mask


def fused_site(mult: float):
    """ita_debug_fused_site: the load-time search for an accumulator base C (an int32 pattern near ACC_BIAS) and the constant K
    with which one fma(C + sum, mult, K) requantises a site like the reference -> (C, K), or None when no candidate passes
    the enumeration or mult is out of range (host only: no GPU, no handle)"""
    c, k = C.c_int(0), C.c_float(0.0)
    if not lib().ita_debug_fused_site(C.c_float(float(mult)), C.byref(c), C.byref(k)):
        return None
    return c.value, k.value


def fused_check(mult: float, base: int, logits: bool = False, relu: bool = False, dq: bool = False):
    """ita_debug_fused_check: the enumeration alone, on a given base -> (accepted, K); logits: the 16-bit travel form of
    the logits, relu: fc1's form (codes 0 .. 127), dq: the dequantise form of out_proj and fc2 (float clamp to [-128, 127])"""
    k = C.c_float(0.0)
    ok = lib().ita_debug_fused_check(C.c_float(float(mult)), 3 if dq else 1 if logits else 2 if relu else 0, int(base), C.byref(k))
    return bool(ok), k.value


DQ_SITES = ("O", "fc2")    # bits 6 and 7 of the fused mask: the fused dequantise form


def dequant_site(mult: float, dmax: int = 1 << 18):
    """ita_debug_dequant_site: the search of the fused dequantise form, the base within dmax of ACC_BIAS -> (C, K) or None"""
    c, k = C.c_int(0), C.c_float(0.0)
    if not lib().ita_debug_dequant_site(C.c_float(float(mult)), int(dmax), C.byref(c), C.byref(k)):
        return None
    return c.value, k.value


class Engine:
    """One ita_context: weights resident on one GPU, stateless compute calls on caller-owned tensors."""

    def __init__(self, blob: bytes, device: Optional[int] = None, reserve: int = 0):
        torch = _torch()
        if not torch.cuda.is_available():
            raise ITAError("no GPU visible: the ITA engine has no CPU path")
        self.device = torch.cuda.current_device() if device is None else int(device)
        self._h = C.c_void_p()
        _chk(lib().ita_create(C.byref(self._h), self.device))
        self.load_weights(blob)
        self._reserved = 0          # frames the workspace is pinned for (ita_reserve); grows only
        self._graphs = []           # weakrefs of live captured graphs: they hold raw workspace pointers
        if reserve:
            self.reserve(reserve)

    def load_weights(self, blob: bytes):
        """(Re)load a blob into this handle (ita_load_weights) and read its dims.  A refused blob raises and leaves the
        handle without weights: load another one."""
        buf = C.create_string_buffer(blob, len(blob))
        _chk(lib().ita_load_weights(self._h, buf, len(blob)))
        d = [C.c_int() for _ in range(6)]
        _chk(lib().ita_get_dims(self._h, *[C.byref(x) for x in d]))
        self.E, self.S, self.P, self.F, self.H, self.num_layers = [x.value for x in d]

    def reserve(self, batch: int):
        """Size and pin the workspace for `batch` frames (ita_reserve).  Growing it frees and reallocates every internal
        buffer, which would leave a HIP graph captured earlier on this engine replaying freed pointers: refused while
        such a graph is alive (build the largest graph first, or use one Engine per batch size)."""
        batch = int(batch)
        if batch <= self._reserved:
            return
        self._graphs = [g for g in self._graphs if g() is not None]
        if self._graphs:
            raise ITAError(f"reserve({batch}) would reallocate the workspace (pinned for {self._reserved} frames) under "
                           f"{len(self._graphs)} live captured graph(s) of this engine: delete them first, or create the "
                           "engine with reserve= the largest batch")
        _chk(lib().ita_reserve(self._h, batch))
        self._reserved = batch

    def _track_graph(self, g):
        import weakref
        self._graphs.append(weakref.ref(g))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            lib().ita_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- int8 blocks -------------------------------------------------------------------
    def mha(self, x, layer: int = 0, taps: bool = False):
        """the layer's attention block without residual / LayerNorm: ITASelfAttention_QAT.forward, (B,128,E) f32 ->
        (B,128,E) f32 [, dict of int tensors], or, on an ITAW0003 blob, the float32 ITASelfAttention (no taps).  The
        logits and probs taps are (B,128,128) at one head and (B,H,128,128) at H > 1."""
        torch = _torch()
        if self.attn_kind(layer) == ATTN_F32:
            if taps:
                raise ITAError("a float32 attention layer has no int8 taps")
            return self.mha_f32(x, layer)
        x = _dev_f32(x)
        B = x.shape[0]
        y = torch.empty_like(x)
        if not taps:
            _chk(lib().ita_mha_int8(self._h, layer, x.data_ptr(), y.data_ptr(), B, _stream_ptr(self.device)))
            return y
        mk = lambda *s, dt=torch.int8: torch.empty(s, dtype=dt, device=x.device)
        lp = (B, 128, 128) if self.H == 1 else (B, self.H, 128, 128)
        t = dict(x_q=mk(B, 128, self.E), Q=mk(B, 128, self.P), K=mk(B, 128, self.P), V=mk(B, 128, self.P),
                 logits=mk(*lp), probs=mk(*lp, dt=torch.uint8), ctx=mk(B, 128, self.P),
                 out_q=mk(B, 128, self.E))
        st = _MhaTaps(**{k: v.data_ptr() for k, v in t.items()})
        _chk(lib().ita_mha_int8_taps(self._h, layer, x.data_ptr(), y.data_ptr(), B, C.byref(st), _stream_ptr(self.device)))
        return y, t

    def layer_forms(self, layer: int = 0) -> dict:
        """ita_debug_layer_forms: which requantisation form and which kernels the layer runs -> fast_sites (the
        ITA_SITE_* mask, bits 0..5 = Q, K, V, logits, context, out_proj), fast (all six sites proven: the stream kernels run their single-rounding instantiation),
        attn_image (mha without taps, mha_q8 and the long entries run on the stream kernels; else block kernels or a
        refusal), layer_image (encoder_layer is one stream-kernel launch), tok_image"""
        m, im = C.c_uint(0), C.c_int(0)
        _chk(lib().ita_debug_layer_forms(self._h, layer, C.byref(m), C.byref(im)))
        return dict(fast_sites=m.value, fast=m.value == 63, attn_image=bool(im.value & FORMS_ATTN_IMAGE),
                    layer_image=bool(im.value & FORMS_LAYER_IMAGE), tok_image=bool(im.value & FORMS_TOK_IMAGE))

    def layer_fused(self, layer: int = 0) -> dict:
        """ita_debug_layer_fused: fused_sites (bits 0..5 = Q, K, V, logits, context, fc1: proven, and not turned off by
        ITA_FUSED_SITES), fused (the stream kernels run their one-fma instantiation on this layer), fused_relu (the
        whole-layer flavours run fc1's fused ReLU form too), C and K per site"""
        m, f = C.c_uint(0), C.c_int(0)
        c6, k6 = (C.c_int * 6)(), (C.c_float * 6)()
        _chk(lib().ita_debug_layer_fused(self._h, layer, C.byref(m), C.byref(f), c6, k6))
        return dict(fused_sites=m.value, fused=f.value >= 1, fused_relu=f.value == 2, C=list(c6), K=list(k6))

    def layer_dequant(self, layer: int = 0) -> dict:
        """ita_debug_layer_dequant: fused_dq (the whole-layer flavours run the fused dequantise form at out_proj and fc2),
        and their C and K"""
        f = C.c_int(0)
        c2, k2 = (C.c_int * 2)(), (C.c_float * 2)()
        _chk(lib().ita_debug_layer_dequant(self._h, layer, C.byref(f), c2, k2))
        return dict(fused_dq=bool(f.value), C=list(c2), K=list(k2))

    def fill_x2_planes(self, batch: int, byte: int):
        """ita_debug_x2_planes: set every byte of the first `batch` rows of both x2 planes, padding included"""
        _chk(lib().ita_debug_x2_planes(self._h, int(byte) & 0xff or 1, None, None, batch, None, _stream_ptr(self.device)))

    def x2_planes(self, batch: int):
        """ita_debug_x2_planes: (hi, lo) f16 tensors (batch, ld_planes): the planes the encoder handed to the folded GEMM"""
        torch = _torch()
        ld = C.c_int(0)
        lib().ita_debug_x2_planes(self._h, 1, None, None, 0, C.byref(ld), None)   # (refused for batch 0; reports the stride)
        hi = torch.empty((batch, ld.value), dtype=torch.float16, device=f"cuda:{self.device}")
        lo = torch.empty_like(hi)
        _chk(lib().ita_debug_x2_planes(self._h, 0, hi.data_ptr(), lo.data_ptr(), batch, None, _stream_ptr(self.device)))
        return hi, lo

    def attn_kind(self, layer: int = 0) -> int:
        """ATTN_INT8 (ITAW0001 / ITAW0002 blob) or ATTN_F32 (ITAW0003: the float graph's float32 attention)"""
        k = C.c_int(-1)
        _chk(lib().ita_get_attn_kind(self._h, layer, C.byref(k)))
        return k.value

    def head_status(self) -> int:
        """device status of the LSTM head since the last query: 0, or HEAD_TIMEOUT (that call's outputs are invalid; the
        head is re-armed).  Waits for the device."""
        st = C.c_int(-1)
        _chk(lib().ita_head_status(self._h, C.byref(st)))
        return st.value

    def mha_f32(self, x, layer: int = 0):
        """ITASelfAttention.forward (float32, softmax(Q K^T) V, no residual / LayerNorm) of a float-attention layer:
        (B,128,E) f32 -> (B,128,E) f32"""
        x = _dev_f32(x)
        y = _torch().empty_like(x)
        _chk(lib().ita_mha_f32(self._h, layer, x.data_ptr(), y.data_ptr(), x.shape[0], _stream_ptr(self.device)))
        return y

    def ffn_kind(self, layer: int = 0) -> int:
        """FFN_INT8 (ITAW0001 blob) or FFN_F32 (ITAW0002: the attention-only graph's float32 FFN)"""
        k = C.c_int(-1)
        _chk(lib().ita_get_ffn_kind(self._h, layer, C.byref(k)))
        return k.value

    def ffn_f32(self, x, layer: int = 0):
        """ITAFeedForward.forward (float32, no residual / LayerNorm) of a float-FFN layer: (B,128,E) f32 -> (B,128,E) f32"""
        x = _dev_f32(x)
        y = _torch().empty_like(x)
        _chk(lib().ita_ffn_f32(self._h, layer, x.data_ptr(), y.data_ptr(), x.shape[0], _stream_ptr(self.device)))
        return y

    def ffn(self, x, layer: int = 0, taps: bool = False):
        """the layer's FFN block without residual / LayerNorm: ITAFeedForward_QAT (int8; taps: its int8 tensors) or, on
        an ITAW0002 blob, the float32 ITAFeedForward (no taps)"""
        torch = _torch()
        if self.ffn_kind(layer) == FFN_F32:
            if taps:
                raise ITAError("a float32 FFN layer has no int8 taps")
            return self.ffn_f32(x, layer)
        x = _dev_f32(x)
        B = x.shape[0]
        y = torch.empty_like(x)
        if not taps:
            _chk(lib().ita_ffn_int8(self._h, layer, x.data_ptr(), y.data_ptr(), B, _stream_ptr(self.device)))
            return y
        mk = lambda *s: torch.empty(s, dtype=torch.int8, device=x.device)
        t = dict(x_q=mk(B, 128, self.E), h=mk(B, 128, self.F), out_q=mk(B, 128, self.E))
        st = _FfnTaps(**{k: v.data_ptr() for k, v in t.items()})
        _chk(lib().ita_ffn_int8_taps(self._h, layer, x.data_ptr(), y.data_ptr(), B, C.byref(st), _stream_ptr(self.device)))
        return y, t

    def encoder_layer(self, x, layer: int = 0):
        x = _dev_f32(x)
        y = _torch().empty_like(x)
        _chk(lib().ita_encoder_layer(self._h, layer, x.data_ptr(), y.data_ptr(), x.shape[0], _stream_ptr(self.device)))
        return y

    # ---- float stages ------------------------------------------------------------------
    def tokenizer(self, img):
        torch = _torch()
        img, dt = self._image(img)
        B = img.shape[0]
        tok = torch.empty((B, 128, self.E), dtype=torch.float32, device=img.device)
        _chk(lib().ita_tokenizer(self._h, img.data_ptr(), dt, tok.data_ptr(), B, _stream_ptr(self.device)))
        return tok

    def fusion_tail(self, x):
        torch = _torch()
        x = _dev_f32(x)
        feat = torch.empty((x.shape[0], 4608), dtype=torch.float32, device=x.device)
        _chk(lib().ita_fusion_tail(self._h, x.data_ptr(), feat.data_ptr(), x.shape[0], _stream_ptr(self.device)))
        return feat

    def _image(self, img):
        torch = _torch()
        if not img.is_cuda:
            raise ITAError("image must be a GPU tensor")
        if img.device.index != self.device:
            raise ITAError(f"tensor lives on cuda:{img.device.index}, the engine on cuda:{self.device}")
        if img.dtype == torch.uint8:
            if tuple(img.shape[-2:]) != (60, 90):   # wire frames are exactly 60 x 90 (ita_wire.h); no silent re-framing
                raise ITAError(f"u8 wire frames must be (..., 60, 90), got {tuple(img.shape)}")
            img = img.reshape(-1, 60, 90).contiguous()
            return img, IMAGE_U8
        img = img.float()
        if img.shape[-2:] != (60, 90):   # refine_inputs: bilinear resize, align_corners=False (QAT/model.py:29-30)
            img = torch.nn.functional.interpolate(img.reshape(-1, 1, *img.shape[-2:]), size=(60, 90),
                                                  mode="bilinear", align_corners=False)
        return img.reshape(-1, 60, 90).contiguous(), IMAGE_F32

    # ---- ingest: camera-resolution frames -> (N,60,90) f32 --------------------------------
    @staticmethod
    def _frame_strides(t):
        """(row_stride, frame_stride) in pixels when the (..., H, W) tensor can be walked as it lies -- last dimension
        dense, leading dimensions collapsing to one frame stride, frames not overlapping -- else None"""
        H, W = int(t.shape[-2]), int(t.shape[-1])
        st = t.stride()
        if W > 1 and st[-1] != 1:
            return None
        rs = int(st[-2]) if H > 1 else W
        if rs < W:
            return None
        extent = (H - 1) * rs + W
        lead = [(int(d), int(s)) for d, s in zip(t.shape[:-2], st[:-2]) if d != 1]
        if not lead:
            return rs, extent
        for (_, s0), (d1, s1) in zip(lead, lead[1:]):
            if s0 != s1 * d1:
                return None
        return (rs, lead[-1][1]) if lead[-1][1] >= extent else None

    def _camera_frames(self, frames, depth_scale, what):
        """the frames argument of ingest and tokenize_long -> (tensor to read, pixel dtype, H, W, N, (row stride, frame
        stride) in pixels, depth_scale): a view that can be walked as it lies is kept, anything else made contiguous"""
        torch = _torch()
        if not hasattr(frames, "is_cuda") or not frames.is_cuda:
            raise ITAError("frames must be a GPU tensor (no CPU fallback)")
        if frames.device.index != self.device:
            raise ITAError(f"tensor lives on cuda:{frames.device.index}, the engine on cuda:{self.device}")
        kinds = {torch.uint8: PIXEL_U8, torch.uint16: PIXEL_U16, torch.int16: PIXEL_U16, torch.float32: PIXEL_F32}
        if frames.dtype not in kinds:
            raise ITAError(f"{what} takes uint8, uint16, int16 or float32 frames, got {frames.dtype}")
        if frames.dim() < 2:
            raise ITAError(f"frames must be (..., H, W), got {tuple(frames.shape)}")
        H, W = int(frames.shape[-2]), int(frames.shape[-1])
        if not (1 <= H <= INGEST_MAX_DIM and 1 <= W <= INGEST_MAX_DIM):
            raise ITAError(f"H and W must be in [1, {INGEST_MAX_DIM}], got {H} x {W}")
        N = np_prod(frames.shape[:-2])
        if N < 1:
            raise ITAError(f"no frames in a tensor of shape {tuple(frames.shape)}")
        strides = self._frame_strides(frames)
        if strides is None:
            frames = frames.contiguous()
            strides = (W, H * W)
        if depth_scale is None:
            depth_scale = 1.0 / 65535.0
        return frames, kinds[frames.dtype], H, W, N, strides, float(depth_scale)

    def ingest(self, frames, depth_scale: Optional[float] = None, out=None):
        """refine_inputs' resize as a stage of its own (ita_ingest): frames (..., H, W) on this engine's GPU, H and W in
        [1, 4096], uint8 (value code / 255), uint16 or int16 taken as the same bits (value min(code * depth_scale, 1),
        depth_scale default 1 / 65535) or float32 (as is) -> (N,60,90) f32, bilinear with align_corners=False, equal to
        ingest_ref.ingest_reference bit for bit.  A view whose last dimension is dense and whose leading dimensions
        collapse to one frame stride (a cropped camera buffer) is read through its strides without a copy; anything else
        is made contiguous first.  The result is allocated per call, or written into out ((N,60,90) f32, contiguous); hand
        it to forward / forward_sequence / forward_slots as f32 frames: eng.forward(eng.ingest(raw), desvel)."""
        torch = _torch()
        frames, kind, H, W, N, strides, depth_scale = self._camera_frames(frames, depth_scale, "ingest")
        if out is None:
            out = torch.empty((N, 60, 90), dtype=torch.float32, device=frames.device)
        elif not out.is_cuda or out.device.index != self.device or out.dtype != torch.float32 or not out.is_contiguous() \
                or tuple(out.shape) != (N, 60, 90):
            raise ITAError(f"out must be a contiguous f32 tensor of shape ({N}, 60, 90) on cuda:{self.device}")
        _chk(lib().ita_ingest(self._h, frames.data_ptr(), kind, H, W, strides[0], strides[1],
                              float(depth_scale), out.data_ptr(), N, _stream_ptr(self.device)))
        return out

    # ---- wire ingest: camera-resolution u8 frames -> (N,60,90) u8 wire frames --------------
    def prepare_ingest_wire(self, H: int, W: int):
        """ita_ingest_wire_prepare: builds and uploads the filter tables of an H x W source, so that ingest_wire on that
        size allocates nothing (a CUDA-graph capture needs this first).  The engine keeps the last eight sizes."""
        _chk(lib().ita_ingest_wire_prepare(self._h, int(H), int(W)))

    def ingest_wire(self, frames, out=None):
        """The reference host's resize (ita_ingest_wire): frames (..., H, W) uint8 on this engine's GPU, H and W in
        [1, 4096] -> (N,60,90) uint8 wire frames: stb_image_resize2's default filters (Mitchell down, Catmull-Rom up, edge
        clamp), equal to ingest_wire_ref.ingest_wire_reference bit for bit and within 1 code of stb itself.  Strided
        views are read as Engine.ingest reads them.  The result is allocated per call, or written into out ((N,60,90)
        uint8, contiguous); hand it to forward / forward_sequence / forward_slots, which run it on the u8 wire path:
        eng.forward(eng.ingest_wire(raw), desvel)."""
        torch = _torch()
        if not hasattr(frames, "is_cuda") or not frames.is_cuda:
            raise ITAError("frames must be a GPU tensor (no CPU fallback)")
        if frames.device.index != self.device:
            raise ITAError(f"tensor lives on cuda:{frames.device.index}, the engine on cuda:{self.device}")
        if frames.dtype != torch.uint8:
            raise ITAError(f"ingest_wire takes uint8 frames, got {frames.dtype}")
        if frames.dim() < 2:
            raise ITAError(f"frames must be (..., H, W), got {tuple(frames.shape)}")
        H, W = int(frames.shape[-2]), int(frames.shape[-1])
        if not (1 <= H <= INGEST_MAX_DIM and 1 <= W <= INGEST_MAX_DIM):
            raise ITAError(f"H and W must be in [1, {INGEST_MAX_DIM}], got {H} x {W}")
        N = np_prod(frames.shape[:-2])
        if N < 1:
            raise ITAError(f"no frames in a tensor of shape {tuple(frames.shape)}")
        strides = self._frame_strides(frames)
        if strides is None:
            frames = frames.contiguous()
            strides = (W, H * W)
        if out is None:
            out = torch.empty((N, 60, 90), dtype=torch.uint8, device=frames.device)
        elif not out.is_cuda or out.device.index != self.device or out.dtype != torch.uint8 or not out.is_contiguous() \
                or tuple(out.shape) != (N, 60, 90):
            raise ITAError(f"out must be a contiguous uint8 tensor of shape ({N}, 60, 90) on cuda:{self.device}")
        _chk(lib().ita_ingest_wire(self._h, frames.data_ptr(), H, W, strides[0], strides[1], out.data_ptr(), N,
                                   _stream_ptr(self.device)))
        return out

    # ---- whole graph -------------------------------------------------------------------
    def forward(self, img, desvel, quat=None, hidden=None, taps: bool = False, out=None):
        """module.main_graph with a leading batch.  Returns (vel (B,3), (h, c) each (3,B,128))."""
        torch = _torch()
        img, dt = self._image(img)
        B, dev = img.shape[0], img.device
        desvel = _dev_f32(desvel).reshape(B)
        if quat is None:   # refine_inputs default quaternion [1,0,0,0] (QAT/model.py:23-27)
            quat = torch.zeros((B, 4), dtype=torch.float32, device=dev)
            quat[:, 0] = 1
        quat = _dev_f32(quat, (B, 4))
        if hidden is None:
            h_in = torch.zeros((3, B, 128), dtype=torch.float32, device=dev)
            c_in = torch.zeros((3, B, 128), dtype=torch.float32, device=dev)
        else:
            h_in, c_in = _dev_f32(hidden[0], (3, B, 128)), _dev_f32(hidden[1], (3, B, 128))
        if out is None:
            vel = torch.empty((B, 3), dtype=torch.float32, device=dev)
            h_out, c_out = torch.empty_like(h_in), torch.empty_like(c_in)
        else:
            vel, h_out, c_out = out
        tp, st = {}, None
        if taps:
            mk = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
            tp = dict(tokens=mk(B, 128, self.E), x1=mk(B, 128, self.E), x2=mk(B, 128, self.E))
            if getattr(self, "_tail_mode", 1) == 0:   # the folded tail (mode 1) never materialises feat / dec
                tp.update(feat=mk(B, 4608), dec=mk(B, 512))
            st = C.byref(_FwdTaps(**{k: tp[k].data_ptr() if k in tp else None for k in ("tokens", "x1", "x2", "feat", "dec")}))
        _chk(lib().ita_vitlstm_forward(self._h, img.data_ptr(), dt, desvel.data_ptr(), quat.data_ptr(),
                                       h_in.data_ptr(), c_in.data_ptr(), vel.data_ptr(), h_out.data_ptr(),
                                       c_out.data_ptr(), B, st, _stream_ptr(self.device)))
        if taps:
            return vel, (h_out, c_out), tp
        return vel, (h_out, c_out)

    def forward_sequence(self, imgs, desvels, quats=None, hidden=None, lengths=None, out=None):
        """T time steps of B streams in one call (ita_vitlstm_sequence): the image-only part of all T * B frames runs as
        one batch (in chunks of what the workspace holds: reserve T * B frames to avoid seams), the recurrence as one
        kernel launch per chunk.  Equal to T calls of forward, bit for bit.

        imgs (T,B,60,90) u8, or f32 (another size is resized as forward does); desvels (T,B); quats (T,B,4), default
        [1,0,0,0]; hidden (h, c) each (3,B,128), default zero, not modified unless handed back as out; lengths (B) int:
        stream b takes part in the steps t < lengths[b] only -- behind them its state is kept and its rows of vel are
        left untouched.  out = (vel (T,B,3), h, c).  Returns (vel, (h, c)), h and c after the last step.  Needs tail mode 1.
        Measured per step on a 1024-frame workspace (tools/bench_sequence.py): 0.28-0.30 x the best step schedule at 1 and 8
        streams, 0.35 x at 32, 0.50 x at 128; at 1024 streams (one step per chunk) it LOSES to a loop of forward by 12 %."""
        torch = _torch()
        if imgs.dim() != 4:
            raise ITAError(f"imgs must be (T, B, H, W), got {tuple(imgs.shape)}")
        T, B = int(imgs.shape[0]), int(imgs.shape[1])
        img, dt = self._image(imgs)
        dev = img.device
        desvels = _dev_f32(desvels).reshape(T, B)
        if quats is None:
            quats = torch.zeros((T, B, 4), dtype=torch.float32, device=dev)
            quats[..., 0] = 1
        quats = _dev_f32(quats, (T, B, 4))
        if out is None:
            vel = torch.empty((T, B, 3), dtype=torch.float32, device=dev)
            h = torch.empty((3, B, 128), dtype=torch.float32, device=dev)
            c = torch.empty_like(h)
        else:
            vel, h, c = out
            for t, shp in ((vel, (T, B, 3)), (h, (3, B, 128)), (c, (3, B, 128))):
                if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != shp:
                    raise ITAError(f"out tensors must be contiguous f32 GPU tensors of shape (T,B,3), (3,B,128), (3,B,128); got {tuple(t.shape)}")
        if hidden is None:
            h.zero_()
            c.zero_()
        else:
            h_in, c_in = _dev_f32(hidden[0], (3, B, 128)), _dev_f32(hidden[1], (3, B, 128))
            if h_in.data_ptr() != h.data_ptr():
                h.copy_(h_in)
            if c_in.data_ptr() != c.data_ptr():
                c.copy_(c_in)
        lp = None
        if lengths is not None:
            lengths = torch.as_tensor(lengths).to(device=dev, dtype=torch.int32).contiguous()
            if tuple(lengths.shape) != (B,):
                raise ITAError(f"lengths must have shape ({B},), got {tuple(lengths.shape)}")
            lp = lengths.data_ptr()
        _chk(lib().ita_vitlstm_sequence(self._h, img.data_ptr(), dt, desvels.data_ptr(), quats.data_ptr(), h.data_ptr(),
                                        c.data_ptr(), lp, vel.data_ptr(), T, B, _stream_ptr(self.device)))
        return vel, (h, c)

    def mha_q8(self, x_q, layer: int = 0):
        """attention block on int8 codes: x_q (B,128,E) int8 -> out_q (B,128,E) int8 (ita_mha_q8)"""
        torch = _torch()
        assert x_q.dtype == torch.int8 and x_q.is_cuda and tuple(x_q.shape[1:]) == (128, self.E)
        x_q = x_q.contiguous()
        out = torch.empty_like(x_q)
        _chk(lib().ita_mha_q8(self._h, layer, x_q.data_ptr(), out.data_ptr(), x_q.shape[0], _stream_ptr(self.device)))
        return out

    def mha_long_q8(self, x_q, layer: int = 0):
        """attention block on int8 codes over a long sequence: x_q (B,S,E) int8, S a multiple of 128 -> out_q (B,S,E) int8
        (ita_mha_long_q8; BASELINE config 5 as worded: S = 8192)"""
        torch = _torch()
        assert x_q.dtype == torch.int8 and x_q.is_cuda and x_q.dim() == 3 and x_q.shape[2] == self.E
        x_q = x_q.contiguous()
        out = torch.empty_like(x_q)
        _chk(lib().ita_mha_long_q8(self._h, layer, x_q.data_ptr(), out.data_ptr(), x_q.shape[0], x_q.shape[1],
                                   _stream_ptr(self.device)))
        return out

    def _long_f32(self, x):
        if x.dim() != 3 or x.shape[2] != self.E:
            raise ITAError(f"expected (B, S, {self.E}) tokens, got {tuple(x.shape)}")
        return _dev_f32(x)

    def mha_long(self, x, layer: int = 0):
        """attention block over a long sequence: x (B,S,E) f32, S a multiple of 128 -> attn(x) (B,S,E) f32
        (ita_mha_long_int8: the long form of mha)"""
        torch = _torch()
        x = self._long_f32(x)
        y = torch.empty_like(x)
        _chk(lib().ita_mha_long_int8(self._h, layer, x.data_ptr(), y.data_ptr(), x.shape[0], x.shape[1],
                                     _stream_ptr(self.device)))
        return y

    def _long_taps(self, x, rows, layer, want):
        """ita_mha_long_int8_taps asking for the taps named in `want` only -> (y, dict of those taps)"""
        torch = _torch()
        x = self._long_f32(x)
        B, S = x.shape[0], x.shape[1]
        rows = [int(r) for r in rows]
        n = len(rows)
        y = torch.empty_like(x)
        i8, u8, i32 = torch.int8, torch.uint8, torch.int32
        spec = dict(x_q=((B, S, self.E), i8), Q=((B, S, self.P), i8), K=((B, S, self.P), i8), V=((B, S, self.P), i8),
                    ctx=((B, S, self.P), i8), out_q=((B, S, self.E), i8), logits=((B, n, S), i8), probs=((B, n, S), u8),
                    row_max=((B, n), i8), row_sum=((B, n), i32))
        unknown = [k for k in want if k not in spec]
        if unknown:
            raise ITAError(f"no such long tap: {unknown}")
        t = {k: torch.empty(spec[k][0], dtype=spec[k][1], device=x.device) for k in spec if k in want}
        st = _MhaLongTaps(**{k: v.data_ptr() for k, v in t.items()})
        arr = (C.c_int * max(n, 1))(*rows)
        st.rows, st.n_rows = (arr if n else None), n
        _chk(lib().ita_mha_long_int8_taps(self._h, layer, x.data_ptr(), y.data_ptr(), B, S, C.byref(st),
                                          _stream_ptr(self.device)))
        return y, t

    def mha_long_taps(self, x, rows=(), layer: int = 0):
        """mha_long with its int tensors read out (ita_mha_long_int8_taps): x (B,S,E) f32 -> (attn(x), taps).  taps: x_q,
        out_q (B,S,E) int8; Q, K, V, ctx (B,S,P) int8; and, for the query rows `rows` (strictly increasing token
        indices, at most 1024, the same of every frame): logits (B,n,S) int8, probs (B,n,S) uint8, row_max (B,n) int8,
        row_sum (B,n) int32.  Without rows the dict holds the six tensors only.  The taps are the long kernels' own values."""
        rows = list(rows)
        return self._long_taps(x, rows, layer, LONG_TENSOR_TAPS + (LONG_ROW_TAPS if rows else ()))

    def attention_rows_long(self, x, rows, layer: int = 0):
        """what the tokens `rows` of a long sequence attend to: x (B,S,E) f32 -> the integer softmax's uint8 probabilities
        (B, len(rows), S) of those query rows (the reference's attn_weights); rows strictly increasing, at most 1024"""
        return self._long_taps(x, rows, layer, ("probs",))[1]["probs"]

    def attention_map_long(self, frames, tok_h: int, tok_w: int, queries, layer: int = 0, depth_scale: Optional[float] = None):
        """attention maps of chosen tokens over the token grid of camera frames: tokenize_long, the encoder layers below
        `layer` (encoder_layer_long, or encoder_layer_long_f32 where the layer's FFN is float), then attention_rows_long of
        `layer` for the tokens queries = [(ty, tx), ...] -> (N, len(queries), tok_h, tok_w) uint8 in the order of queries.
        Duplicate or out-of-grid queries raise ValueError."""
        return self._attention_map_walk(frames, tok_h, tok_w, queries, layer, depth_scale, self.attention_rows_long)

    def _long_stats(self, x, layer, want):
        """ita_mha_long_int8_stats asking for the statistics named in `want` only -> dict of those"""
        torch = _torch()
        x = self._long_f32(x)
        B, S = x.shape[0], x.shape[1]
        unknown = [k for k in want if k not in LONG_STATS]
        if unknown:
            raise ITAError(f"no such long statistic: {unknown}")
        t = {k: torch.empty((B, S), dtype=torch.int8 if k == "row_max" else torch.int32, device=x.device)
             for k in LONG_STATS if k in want}
        st = _MhaLongStats(**{k: v.data_ptr() for k, v in t.items()})
        _chk(lib().ita_mha_long_int8_stats(self._h, layer, x.data_ptr(), B, S, C.byref(st), _stream_ptr(self.device)))
        return t

    def attention_stats_long(self, x, layer: int = 0):
        """row and column statistics of the whole S x S integer-softmax matrix of a long sequence, which is never held
        (ita_mha_long_int8_stats): x (B,S,E) f32 -> dict of (B,S) tensors.  Per query row: row_max int8, row_sum int32 (as
        mha_long_taps has them), row_mass int32 = sum of the row's uint8 probabilities (256 if nothing was lost, 0 for a row
        the integer softmax killed), row_nnz int32 = keys the row still sees.  Per key: col_mass int32 = attention received
        from all queries, col_nnz int32 = queries that see the key.  Equal to attention_stats_ref.stats."""
        return self._long_stats(x, layer, LONG_STATS)

    def attention_received_long(self, x, layer: int = 0):
        """attention received by every token of a long sequence: x (B,S,E) f32 -> col_mass (B,S) int32, the column sums
        of the uint8 probabilities over all S queries"""
        return self._long_stats(x, layer, ("col_mass",))["col_mass"]

    def attention_received_map_long(self, frames, tok_h: int, tok_w: int, layer: int = 0, depth_scale: Optional[float] = None):
        """attention received on the token grid of camera frames: tokenize_long, the encoder layers below `layer`, then
        attention_received_long of `layer` -> (N, tok_h, tok_w) int32"""
        y = self._tokens_below(frames, int(tok_h), int(tok_w), layer, depth_scale)
        return self.attention_received_long(y, int(layer)).reshape(y.shape[0], int(tok_h), int(tok_w))

    def _long_hist(self, x, layer, want):
        """ita_mha_long_int8_hist asking for the outputs named in `want` only -> dict of those"""
        torch = _torch()
        x = self._long_f32(x)
        B, S = x.shape[0], x.shape[1]
        unknown = [k for k in want if k not in LONG_HIST]
        if unknown:
            raise ITAError(f"no such long histogram: {unknown}")
        spec = dict(logits=((B, 256), torch.int64), logits_out=((B, 2), torch.int64), acc_range=((B, 2), torch.int32),
                    shifts=((B, 256), torch.int64), probs=((B, 256), torch.int64))
        t = {k: torch.empty(spec[k][0], dtype=spec[k][1], device=x.device) for k in LONG_HIST if k in want}
        st = _MhaLongHist(**{k: v.data_ptr() for k, v in t.items()})
        _chk(lib().ita_mha_long_int8_hist(self._h, layer, x.data_ptr(), B, S, C.byref(st), _stream_ptr(self.device)))
        return t

    def attention_histograms_long(self, x, layer: int = 0, stages: bool = False):
        """histograms of the whole S x S matrix of a long sequence in front of and behind the integer softmax, which is
        never held (ita_mha_long_int8_hist): x (B,S,E) f32 -> dict of logits (B,256) int64 (bin c + 128 counts the int8
        logit c), logits_out (B,2) int64 (raw logits below -128 and above 127: what the clamp changed), acc_range (B,2)
        int32 (minimum and maximum of the Q K^T accumulators), shifts (B,256) int64 (row maximum - logit; the softmax
        resolves 0 .. 15) and probs (B,256) int64 (the uint8 probabilities).  Equal to attention_hist_ref.hist.  With
        stages=True also (B,256) int64 histograms (bin c + 128) of the int8 stage tensors x_q, Q, K, V, ctx and out_q of
        mha_long_taps, counted with torch."""
        torch = _torch()
        out = self._long_hist(x, layer, LONG_HIST)
        if stages:
            _, taps = self._long_taps(x, (), layer, LONG_HIST_STAGES)
            for k in LONG_HIST_STAGES:
                v = taps[k].reshape(taps[k].shape[0], -1).to(torch.int64) + 128
                out[k] = torch.stack([torch.bincount(r, minlength=256) for r in v])
        return out

    def attention_histograms_frames_long(self, frames, tok_h: int, tok_w: int, layer: int = 0, depth_scale: Optional[float] = None):
        """the histograms of attention_histograms_long for camera frames: tokenize_long, the encoder layers below `layer`,
        then attention_histograms_long of `layer` -> its dict"""
        y = self._tokens_below(frames, int(tok_h), int(tok_w), layer, depth_scale)
        return self.attention_histograms_long(y, int(layer))

    def attention_propagate_long(self, x, w, layer: int = 0):
        """weighted column sums of the whole S x S integer-softmax matrix of a long sequence, which is never held
        (ita_mha_long_int8_propagate): x (B,S,E) f32, w int8 GPU tensor (B,R,S), or (R,S) for the same weights of every
        frame (copied B times), 1 <= R <= 64 -> out (B,R,S) int32, out[b,r,j] = sum_i w[b,r,i] p[b,i,j] with p the uint8
        probabilities of attention_rows_long.  Exact: equal to attention_propagate_ref.propagate.  All-ones weights give
        attention_received_long, a one-hot row gives that probability row.  Every partial sum fits int32 for any int8
        weight at S <= 32768 and at S = 65536 for weights in [-127, 127] (127 * 128 * 65536 < 2^30, twice); the weights
        are not scanned."""
        torch = _torch()
        x = self._long_f32(x)
        B, S = x.shape[0], x.shape[1]
        if not w.is_cuda or w.dtype != torch.int8 or w.dim() not in (2, 3) or w.shape[-1] != S or (w.dim() == 3 and w.shape[0] != B):
            raise ITAError(f"w must be an int8 GPU tensor of shape ({B}, R, {S}) or (R, {S}), got {w.dtype} {tuple(w.shape)}")
        if w.dim() == 2:
            w = w.unsqueeze(0).expand(B, -1, -1)
        w = w.contiguous()
        out = torch.empty((B, w.shape[1], S), dtype=torch.int32, device=x.device)
        _chk(lib().ita_mha_long_int8_propagate(self._h, layer, x.data_ptr(), B, S, w.data_ptr(), w.shape[1], out.data_ptr(),
                                               _stream_ptr(self.device)))
        return out

    def attention_rollout_long(self, x, rows=None, first_layer: int = 0):
        """attention rollout (Abnar & Zuidema) through the int8 attention layers first_layer .. num_layers - 1 of a long
        sequence: identity residual, attention matrix P_l / 256.  x (B,S,E) f32: the token rows entering first_layer;
        rows: token indices in any order (duplicates raise ValueError), or None for the single start vector 1 / S ->
        (B, n, S) float64 on x's device: how much output token rows[n] depends on every input token.  The layers run out
        of place (encoder_layer_long, or encoder_layer_long_f32 where the FFN is float) and each layer's input is kept;
        from the last layer down, with v = one-hot(rows) at the start,
            s = max_j v (1 where that is 0);  q = rint((v / s) * 2097151)
            v <- 0.5 * (v + ((float64(q . P_l) * (s / 2097151)) / 256))
        where q . P_l comes from attention_propagate_long on the three base-128 digit rows of q (rollout_digits,
        rollout_combine): 21 vectors per call, more in chunks.  Equal to attention_rollout_ref.rollout bit for bit."""
        import numpy as np
        torch = _torch()
        x = self._long_f32(x)
        B, S = x.shape[0], x.shape[1]
        first_layer = int(first_layer)
        if not 0 <= first_layer < self.num_layers:
            raise ValueError(f"first_layer {first_layer} out of range")
        if rows is None:
            v = np.full((B, 1, S), 1.0 / S, np.float64)
        else:
            rows = [int(r) for r in rows]
            if any(not 0 <= r < S for r in rows):
                raise ValueError(f"rows must be token indices in [0, {S})")
            if len(set(rows)) != len(rows):
                raise ValueError("duplicate rows")
            v = np.zeros((B, len(rows), S), np.float64)
            for n, r in enumerate(rows):
                v[:, n, r] = 1.0
        xs = [x]
        for l in range(first_layer, self.num_layers - 1):
            step = self.encoder_layer_long_f32 if self.ffn_kind(l) == FFN_F32 else self.encoder_layer_long
            xs.append(step(xs[-1], l))
        for l in range(self.num_layers - 1, first_layer - 1, -1):
            s = v.max(-1, keepdims=True)
            s = np.where(s == 0, 1.0, s)
            q = np.rint((v / s) * float(ROLLOUT_QMAX)).astype(np.int64)
            qp = np.empty(v.shape, np.int64)
            for c0 in range(0, v.shape[1], ROLLOUT_CHUNK):
                c = slice(c0, min(c0 + ROLLOUT_CHUNK, v.shape[1]))
                d = torch.from_numpy(rollout_digits(q[:, c])).to(x.device)
                qp[:, c] = rollout_combine(self.attention_propagate_long(xs[l - first_layer], d, l).cpu().numpy())
            v = 0.5 * (v + ((qp.astype(np.float64) * (s / float(ROLLOUT_QMAX))) / 256.0))
        return torch.from_numpy(v).to(x.device)

    def attention_rollout_map_long(self, frames, tok_h: int, tok_w: int, queries=None, depth_scale: Optional[float] = None):
        """attention rollout on the token grid of camera frames: tokenize_long, then attention_rollout_long through every
        layer for the tokens queries = [(ty, tx), ...] (None: the single start vector 1 / S) -> (N, n, tok_h, tok_w)
        float64 in the order of queries.  Duplicate or out-of-grid queries raise ValueError."""
        tok_h, tok_w = int(tok_h), int(tok_w)
        toks = None
        if queries is not None:
            toks = []
            for ty, tx in queries:
                ty, tx = int(ty), int(tx)
                if not (0 <= ty < tok_h and 0 <= tx < tok_w):
                    raise ValueError(f"query ({ty}, {tx}) lies outside the {tok_h} x {tok_w} token grid")
                toks.append(ty * tok_w + tx)
            if len(set(toks)) != len(toks):
                raise ValueError("duplicate queries")
        y = self.tokenize_long(frames, tok_h, tok_w, depth_scale)
        v = self.attention_rollout_long(y, toks)
        return v.reshape(v.shape[0], v.shape[1], tok_h, tok_w)

    def _tokens_below(self, frames, tok_h, tok_w, layer, depth_scale):
        """tokenize_long and the encoder layers below `layer`: the token rows that layer's attention reads"""
        if not 0 <= int(layer) < self.num_layers:
            raise ValueError(f"layer {layer} out of range")
        y = self.tokenize_long(frames, tok_h, tok_w, depth_scale)
        for l in range(int(layer)):
            if self.ffn_kind(l) == FFN_F32:
                self.encoder_layer_long_f32(y, l, out=y)
            else:
                self.encoder_layer_long(y, l, out=y)
        return y

    def _attention_map_walk(self, frames, tok_h, tok_w, queries, layer, depth_scale, rows_fn):
        """what attention_map_long and attention_map_long_f32 share: the query checks, the walk below `layer`
        (_tokens_below), rows_fn(tokens, sorted token indices, layer) and the un-sorting into the order of queries"""
        tok_h, tok_w = int(tok_h), int(tok_w)
        toks = []
        for ty, tx in queries:
            ty, tx = int(ty), int(tx)
            if not (0 <= ty < tok_h and 0 <= tx < tok_w):
                raise ValueError(f"query ({ty}, {tx}) lies outside the {tok_h} x {tok_w} token grid")
            toks.append(ty * tok_w + tx)
        if len(set(toks)) != len(toks):
            raise ValueError("duplicate queries")
        y = self._tokens_below(frames, tok_h, tok_w, layer, depth_scale)
        order = sorted(range(len(toks)), key=toks.__getitem__)
        probs = rows_fn(y, [toks[j] for j in order], int(layer))
        unsort = [0] * len(order)
        for pos, j in enumerate(order):
            unsort[j] = pos
        torch = _torch()
        probs = probs[:, torch.tensor(unsort, dtype=torch.long, device=probs.device)] if toks else probs
        return probs.reshape(probs.shape[0], len(toks), tok_h, tok_w)

    def encoder_layer_long(self, x, layer: int = 0, out=None):
        """one encoder layer over a long sequence: x (B,S,E) f32 -> LN2(x1 + ffn(x1)), x1 = LN1(x + attn(x))
        (ita_encoder_layer_long); out: optional contiguous f32 GPU tensor of x's shape, may be x itself"""
        torch = _torch()
        x = self._long_f32(x)
        if out is None:
            out = torch.empty_like(x)
        elif not out.is_cuda or out.dtype != torch.float32 or not out.is_contiguous() or out.shape != x.shape:
            raise ITAError(f"out must be a contiguous f32 GPU tensor of shape {tuple(x.shape)}")
        _chk(lib().ita_encoder_layer_long(self._h, layer, x.data_ptr(), out.data_ptr(), x.shape[0], x.shape[1],
                                          _stream_ptr(self.device)))
        return out

    def encode_long(self, x):
        """all num_layers encoder layers in order over a long sequence: (B,S,E) f32 -> (B,S,E) f32"""
        y = self.encoder_layer_long(x, 0)
        for layer in range(1, self.num_layers):
            self.encoder_layer_long(y, layer, out=y)
        return y

    def tokenize_long(self, frames, tok_h: int, tok_w: int, depth_scale: Optional[float] = None, out=None):
        """OverlapPatchMerging for any frame size and token grid (ita_tokenizer_long): frames (..., H, W) on this engine's
        GPU, H and W in [1, 4096], uint8 / uint16 / int16 / float32 valued and read through their strides exactly as
        ingest does -> (N, tok_h * tok_w, E) f32 token rows, the input of mha_long / encoder_layer_long / encode_long and
        FusionTailLarge.  tok_w a multiple of 16, tok_h * tok_w a multiple of 128 up to 65536.  Equal to
        tokenizer_long_ref (blend_patches + the fmaf chain + LayerNorm) bit for bit.  The result is allocated per call, or
        written into out ((N, tok_h * tok_w, E) f32, contiguous)."""
        torch = _torch()
        frames, kind, H, W, N, strides, depth_scale = self._camera_frames(frames, depth_scale, "tokenize_long")
        tok_h, tok_w = int(tok_h), int(tok_w)
        shape = (N, tok_h * tok_w, self.E)
        if out is None:
            if tok_h < 1 or tok_w < 1:
                raise ITAError(f"token grid must be positive, got {tok_h} x {tok_w}")
            out = torch.empty(shape, dtype=torch.float32, device=frames.device)
        elif not out.is_cuda or out.device.index != self.device or out.dtype != torch.float32 or not out.is_contiguous() \
                or tuple(out.shape) != shape:
            raise ITAError(f"out must be a contiguous f32 tensor of shape {shape} on cuda:{self.device}")
        _chk(lib().ita_tokenizer_long(self._h, frames.data_ptr(), kind, H, W, strides[0], strides[1], depth_scale,
                                      tok_h, tok_w, out.data_ptr(), N, _stream_ptr(self.device)))
        return out

    def encode_frames_long(self, frames, tok_h: int, tok_w: int, depth_scale: Optional[float] = None):
        """camera frames -> tokens -> every encoder layer: tokenize_long, then all num_layers of encoder_layer_long in
        place on the token buffer; (..., H, W) -> (N, tok_h * tok_w, E) f32"""
        y = self.tokenize_long(frames, tok_h, tok_w, depth_scale)
        for layer in range(self.num_layers):
            self.encoder_layer_long(y, layer, out=y)
        return y

    def mha_long_f32(self, x, layer: int = 0):
        """float32 attention block over a long sequence: x (B,S,E) f32, S a multiple of 128 -> attn(x) (B,S,E) f32
        (ita_mha_long_f32: the long form of mha_f32, for a float-attention layer)"""
        torch = _torch()
        x = self._long_f32(x)
        y = torch.empty_like(x)
        _chk(lib().ita_mha_long_f32(self._h, layer, x.data_ptr(), y.data_ptr(), x.shape[0], x.shape[1],
                                    _stream_ptr(self.device)))
        return y

    def _long_f32_taps(self, x, rows, layer, want):
        """ita_mha_long_f32_taps asking for the taps named in `want` only -> (y, dict of those taps)"""
        torch = _torch()
        x = self._long_f32(x)
        B, S = x.shape[0], x.shape[1]
        rows = [int(r) for r in rows]
        n = len(rows)
        y = torch.empty_like(x)
        spec = dict(Q=(B, S, self.P), K=(B, S, self.P), V=(B, S, self.P), ctx=(B, S, self.P), logits=(B, n, S),
                    probs=(B, n, S), row_max=(B, n), row_sum=(B, n))
        unknown = [k for k in want if k not in spec]
        if unknown:
            raise ITAError(f"no such long float tap: {unknown}")
        t = {k: torch.empty(spec[k], dtype=torch.float32, device=x.device) for k in spec if k in want}
        st = _MhaLongF32Taps(**{k: v.data_ptr() for k, v in t.items()})
        arr = (C.c_int * max(n, 1))(*rows)
        st.rows, st.n_rows = (arr if n else None), n
        _chk(lib().ita_mha_long_f32_taps(self._h, layer, x.data_ptr(), y.data_ptr(), B, S, C.byref(st),
                                         _stream_ptr(self.device)))
        return y, t

    def mha_long_f32_taps(self, x, rows=(), layer: int = 0):
        """mha_long_f32 with its f32 tensors read out (ita_mha_long_f32_taps): x (B,S,E) f32 -> (attn(x), taps).  taps: Q,
        K, V, ctx (B,S,P); and, for the query rows `rows` (strictly increasing token indices, at most 1024, the same of
        every frame): logits, probs (B,n,S), row_max, row_sum (B,n).  Without rows the dict holds the four tensors only.
        Every tap is the long kernels' own value; probs = ita_expf(logits - row_max) * (1 / row_sum), formed from them."""
        rows = list(rows)
        return self._long_f32_taps(x, rows, layer, LONG_F32_TENSOR_TAPS + (LONG_ROW_TAPS if rows else ()))

    def attention_rows_long_f32(self, x, rows, layer: int = 0):
        """what the tokens `rows` of a long sequence attend to in a float-attention layer: x (B,S,E) f32 -> the softmax
        probabilities (B, len(rows), S) f32 of those query rows; rows strictly increasing, at most 1024"""
        return self._long_f32_taps(x, rows, layer, ("probs",))[1]["probs"]

    def attention_map_long_f32(self, frames, tok_h: int, tok_w: int, queries, layer: int = 0, depth_scale: Optional[float] = None):
        """attention_map_long for a float-attention layer: tokenize_long, the encoder layers below `layer`
        (encoder_layer_long_f32), then attention_rows_long_f32 of `layer` for the tokens queries = [(ty, tx), ...] ->
        (N, len(queries), tok_h, tok_w) f32 in the order of queries.  Duplicate or out-of-grid queries raise ValueError."""
        return self._attention_map_walk(frames, tok_h, tok_w, queries, layer, depth_scale, self.attention_rows_long_f32)

    def _long_f32_stats(self, x, layer, want, p_min):
        """ita_mha_long_f32_stats asking for the statistics named in `want` only -> dict of those"""
        torch = _torch()
        x = self._long_f32(x)
        B, S = x.shape[0], x.shape[1]
        unknown = [k for k in want if k not in LONG_F32_STATS]
        if unknown:
            raise ITAError(f"no such long float statistic: {unknown}")
        t = {k: torch.empty((B, S), dtype=torch.int32 if k.endswith("_nnz") else torch.float32, device=x.device)
             for k in LONG_F32_STATS if k in want}
        st = _MhaLongF32Stats(**{k: v.data_ptr() for k, v in t.items()})
        _chk(lib().ita_mha_long_f32_stats(self._h, layer, x.data_ptr(), B, S, float(p_min), C.byref(st),
                                          _stream_ptr(self.device)))
        return t

    def attention_stats_long_f32(self, x, layer: int = 0, p_min: float = 1.0 / 256):
        """row and column statistics of the whole S x S softmax matrix of a float-attention layer over a long sequence,
        which is never held (ita_mha_long_f32_stats): x (B,S,E) f32 -> dict of (B,S) tensors.  With the probability of
        mha_long_f32_taps, p = ita_expf(logit - row_max) * (1 / row_sum): per query row row_max, row_sum f32 (as the taps
        have them), row_gap f32 = sum_j p (row_max - logit), row_nnz int32 = keys with p >= p_min, and row_entropy f32 =
        log(row_sum) + row_gap, formed here with torch; per key col_mass f32 = attention received from all queries,
        col_nnz int32 = queries with p >= p_min.  The default p_min is about where a uint8 probability of the integer
        softmax stops being zero.  The same input gives the same bits on every call, whatever the batch around a frame.
        Held to attention_stats_f32_ref.stats_from_taps."""
        t = self._long_f32_stats(x, layer, LONG_F32_STATS, p_min)
        t["row_entropy"] = _torch().log(t["row_sum"]) + t["row_gap"]
        return t

    def attention_received_long_f32(self, x, layer: int = 0):
        """attention received by every token of a long sequence in a float-attention layer: x (B,S,E) f32 -> col_mass
        (B,S) f32, the column sums of the probabilities over all S queries"""
        return self._long_f32_stats(x, layer, ("col_mass",), 1.0 / 256)["col_mass"]

    def attention_received_map_long_f32(self, frames, tok_h: int, tok_w: int, layer: int = 0, depth_scale: Optional[float] = None):
        """attention received on the token grid of camera frames in a float-attention layer: tokenize_long, the encoder
        layers below `layer`, then attention_received_long_f32 of `layer` -> (N, tok_h, tok_w) f32"""
        y = self._tokens_below(frames, int(tok_h), int(tok_w), layer, depth_scale)
        return self.attention_received_long_f32(y, int(layer)).reshape(y.shape[0], int(tok_h), int(tok_w))

    def attention_propagate_long_f32(self, x, w, layer: int = 0):
        """weighted column sums of the whole S x S softmax matrix of a float-attention layer over a long sequence, which
        is never held (ita_mha_long_f32_propagate): x (B,S,E) f32, w f32 GPU tensor (B,R,S), or (R,S) for the same weights
        of every frame (copied B times), 1 <= R <= 64 -> out (B,R,S) f32, out[b,r,j] = sum_i w[b,r,i] p[b,i,j] with p the
        probabilities of attention_rows_long_f32.  The f32 sums are taken in one fixed order: a one-hot row gives that
        probability row bit for bit, all-ones weights give attention_received_long_f32 up to the order of the additions,
        a row's bits do not depend on R, its place among the rows or the batch.  Held to
        attention_propagate_f32_ref.propagate_from_taps within gamma_(S+2) sum |w| p.  The weights are not scanned."""
        torch = _torch()
        x = self._long_f32(x)
        B, S = x.shape[0], x.shape[1]
        if not w.is_cuda or w.dtype != torch.float32 or w.dim() not in (2, 3) or w.shape[-1] != S or (w.dim() == 3 and w.shape[0] != B):
            raise ITAError(f"w must be an f32 GPU tensor of shape ({B}, R, {S}) or (R, {S}), got {w.dtype} {tuple(w.shape)}")
        if w.dim() == 2:
            w = w.unsqueeze(0).expand(B, -1, -1)
        w = w.contiguous()
        out = torch.empty((B, w.shape[1], S), dtype=torch.float32, device=x.device)
        _chk(lib().ita_mha_long_f32_propagate(self._h, layer, x.data_ptr(), B, S, w.data_ptr(), w.shape[1], out.data_ptr(),
                                              _stream_ptr(self.device)))
        return out

    def attention_rollout_long_f32(self, x, rows=None, first_layer: int = 0):
        """attention rollout (Abnar & Zuidema) through the float-attention layers first_layer .. num_layers - 1 of a long
        sequence: identity residual, attention matrix P_l of layer l.  x (B,S,E) f32: the token rows entering
        first_layer; rows: token indices in any order (duplicates and out-of-range rows raise ValueError), or None for
        the single start vector 1 / S -> (B, n, S) f32: how much output token rows[n] depends on every input token.  The
        layers run out of place (encoder_layer_long_f32) and each layer's input is kept; from the last layer down, with
        v = one-hot(rows) at the start,
            v <- 0.5 * (v + attention_propagate_long_f32(x_l, v, l))
        the add and the scale in torch f32 on the GPU, 64 vectors per call and more in chunks.  Held to
        attention_rollout_f32_ref.rollout64.  A layer that is not float attention raises ITAError
        (attention_rollout_long walks int8 layers)."""
        torch = _torch()
        x = self._long_f32(x)
        B, S = x.shape[0], x.shape[1]
        first_layer = int(first_layer)
        if not 0 <= first_layer < self.num_layers:
            raise ValueError(f"first_layer {first_layer} out of range")
        for l in range(first_layer, self.num_layers):
            if self.attn_kind(l) != ATTN_F32:
                raise ITAError(f"layer {l} has int8 attention: attention_rollout_long walks int8 layers")
        if rows is None:
            v = torch.full((B, 1, S), 1.0 / S, dtype=torch.float32, device=x.device)
        else:
            rows = [int(r) for r in rows]
            if any(not 0 <= r < S for r in rows):
                raise ValueError(f"rows must be token indices in [0, {S})")
            if len(set(rows)) != len(rows):
                raise ValueError("duplicate rows")
            v = torch.zeros((B, len(rows), S), dtype=torch.float32, device=x.device)
            if rows:
                v[:, torch.arange(len(rows), device=x.device), torch.tensor(rows, dtype=torch.long, device=x.device)] = 1.0
        xs = [x]
        for l in range(first_layer, self.num_layers - 1):
            xs.append(self.encoder_layer_long_f32(xs[-1], l))
        for l in range(self.num_layers - 1, first_layer - 1, -1):
            nxt = torch.empty_like(v)
            for c0 in range(0, v.shape[1], ROLLOUT_F32_CHUNK):
                c = slice(c0, min(c0 + ROLLOUT_F32_CHUNK, v.shape[1]))
                nxt[:, c] = 0.5 * (v[:, c] + self.attention_propagate_long_f32(xs[l - first_layer], v[:, c].contiguous(), l))
            v = nxt
        return v

    def attention_rollout_map_long_f32(self, frames, tok_h: int, tok_w: int, queries=None, depth_scale: Optional[float] = None):
        """attention rollout of a float graph on the token grid of camera frames: tokenize_long, then
        attention_rollout_long_f32 through every layer for the tokens queries = [(ty, tx), ...] (None: the single start
        vector 1 / S) -> (N, n, tok_h, tok_w) f32 in the order of queries.  Duplicate or out-of-grid queries raise
        ValueError."""
        tok_h, tok_w = int(tok_h), int(tok_w)
        toks = None
        if queries is not None:
            toks = []
            for ty, tx in queries:
                ty, tx = int(ty), int(tx)
                if not (0 <= ty < tok_h and 0 <= tx < tok_w):
                    raise ValueError(f"query ({ty}, {tx}) lies outside the {tok_h} x {tok_w} token grid")
                toks.append(ty * tok_w + tx)
            if len(set(toks)) != len(toks):
                raise ValueError("duplicate queries")
        y = self.tokenize_long(frames, tok_h, tok_w, depth_scale)
        v = self.attention_rollout_long_f32(y, toks)
        return v.reshape(v.shape[0], v.shape[1], tok_h, tok_w)

    def encoder_layer_long_f32(self, x, layer: int = 0, out=None):
        """one encoder layer with a float FFN (ITAW0002 / ITAW0003 blob) over a long sequence: x (B,S,E) f32 ->
        LN2(x1 + ffn(x1)), x1 = LN1(x + attn(x)) (ita_encoder_layer_long_f32); out: optional contiguous f32 GPU tensor of
        x's shape, may be x itself"""
        torch = _torch()
        x = self._long_f32(x)
        if out is None:
            out = torch.empty_like(x)
        elif not out.is_cuda or out.dtype != torch.float32 or not out.is_contiguous() or out.shape != x.shape:
            raise ITAError(f"out must be a contiguous f32 GPU tensor of shape {tuple(x.shape)}")
        _chk(lib().ita_encoder_layer_long_f32(self._h, layer, x.data_ptr(), out.data_ptr(), x.shape[0], x.shape[1],
                                              _stream_ptr(self.device)))
        return out

    def encode_long_f32(self, x):
        """all num_layers float-FFN encoder layers in order over a long sequence: (B,S,E) f32 -> (B,S,E) f32"""
        y = self.encoder_layer_long_f32(x, 0)
        for layer in range(1, self.num_layers):
            self.encoder_layer_long_f32(y, layer, out=y)
        return y

    def encode_frames_long_f32(self, frames, tok_h: int, tok_w: int, depth_scale: Optional[float] = None):
        """camera frames -> tokens -> every float-FFN encoder layer: tokenize_long, then all num_layers of
        encoder_layer_long_f32 in place on the token buffer; (..., H, W) -> (N, tok_h * tok_w, E) f32"""
        y = self.tokenize_long(frames, tok_h, tok_w, depth_scale)
        for layer in range(self.num_layers):
            self.encoder_layer_long_f32(y, layer, out=y)
        return y

    def softmax_rows(self, logits):
        """IntegerApproximatedSoftmax through the encoder kernel's own device function: int8 (R,128) -> uint8 (R,128)"""
        torch = _torch()
        assert logits.dtype == torch.int8 and logits.is_cuda and logits.shape[-1] == 128
        lg = logits.reshape(-1, 128).contiguous()
        out = torch.empty(lg.shape, dtype=torch.uint8, device=lg.device)
        _chk(lib().ita_debug_softmax_rows(self._h, lg.data_ptr(), out.data_ptr(), lg.shape[0], _stream_ptr(self.device)))
        return out.reshape(logits.shape)

    def tail(self, x2, desvel, quat, hidden=None):
        """the graph behind the encoder: x2 (B,128,64) -> (vel, (h, c))   (fusion tail, decoder, LSTM, fc)"""
        torch = _torch()
        x2 = _dev_f32(x2)
        B, dev = x2.shape[0], x2.device
        desvel, quat = _dev_f32(desvel).reshape(B), _dev_f32(quat, (B, 4))
        if hidden is None:
            h_in = torch.zeros((3, B, 128), dtype=torch.float32, device=dev)
            c_in = torch.zeros((3, B, 128), dtype=torch.float32, device=dev)
        else:
            h_in, c_in = _dev_f32(hidden[0], (3, B, 128)), _dev_f32(hidden[1], (3, B, 128))
        vel = torch.empty((B, 3), dtype=torch.float32, device=dev)
        h_out, c_out = torch.empty_like(h_in), torch.empty_like(c_in)
        _chk(lib().ita_vitlstm_tail(self._h, x2.data_ptr(), desvel.data_ptr(), quat.data_ptr(), h_in.data_ptr(),
                                    c_in.data_ptr(), vel.data_ptr(), h_out.data_ptr(), c_out.data_ptr(), B,
                                    _stream_ptr(self.device)))
        return vel, (h_out, c_out)

    def encoder_stamps(self, x, layer: int = 0):
        """diagnostic: per-phase s_memtime stamps of the encoder stream kernel -> int64 [blocks, 8 frames, 2 waves
        (0 and 4), 16 slots].  x: (B,128,64) f32 tokens, or (B,60,90) u8 frames (tokenizer fused in front; slots 9, 10)"""
        torch = _torch()
        B = x.shape[0]
        if x.dtype == torch.uint8:
            img, xp = x.reshape(-1, 60, 90).contiguous(), None
        else:
            img, xp = None, _dev_f32(x)
        y = torch.empty((B, 128, self.E), dtype=torch.float32, device=x.device)
        nb = min(B, torch.cuda.get_device_properties(x.device).multi_processor_count)
        st = torch.zeros((nb, 8, 2, 16), dtype=torch.int64, device=x.device)
        _chk(lib().ita_debug_encoder_stamps(self._h, layer, xp.data_ptr() if xp is not None else None,
                                            img.data_ptr() if img is not None else None, y.data_ptr(), B, st.data_ptr(),
                                            _stream_ptr(self.device)))
        return st

    def set_tail_mode(self, mode: int):
        """1: folded conv+decoder, f16x3 split-precision MFMA tail (default); 0: exact f32 kernels"""
        _chk(lib().ita_set_tail_mode(self._h, mode))
        self._tail_mode = mode

    # ---- per-stage device timing ---------------------------------------------------------
    STAGES = ("tokenizer", "mha", "ffn", "tail", "decoder", "lstm_fc")

    def profile_begin(self, max_forwards: int, every_n: int = 1, only_stage: Optional[str] = None):
        """only_stage: one of STAGES -> record only that stage's two events, on every every_n-th forward"""
        st = -1 if only_stage is None else self.STAGES.index(only_stage)
        _chk(lib().ita_profile_begin_sampled(self._h, max_forwards, every_n, st))

    def profile_end(self):
        """-> ({stage: summed ms}, forwards covered)"""
        ms = (C.c_double * 6)()
        n = C.c_int()
        _chk(lib().ita_profile_end(self._h, ms, C.byref(n)))
        return dict(zip(self.STAGES, list(ms))), n.value

    def front(self, img, buf: int, stream=None, encoder_done=None):
        """image-only half of a time step (tokenizer, encoder, folded GEMM) into internal buffer `buf`;
        encoder_done: optional torch.cuda.Event (already recorded once, so that its handle exists) recorded between
        the encoder and the GEMM"""
        img, dt = self._image(img)
        sp = _stream_ptr(self.device) if stream is None else C.c_void_p(stream.cuda_stream)
        ev = None if encoder_done is None else C.c_void_p(encoder_done.cuda_event)
        _chk(lib().ita_vitlstm_front_ev(self._h, img.data_ptr(), dt, img.shape[0], buf, sp, ev))
        return img.shape[0]

    def encode(self, img, plane_set: int, stream=None):
        """tokenizer + encoder of a time step into plane set 0 / 1 (ita_vitlstm_encode)"""
        img, dt = self._image(img)
        sp = _stream_ptr(self.device) if stream is None else C.c_void_p(stream.cuda_stream)
        _chk(lib().ita_vitlstm_encode(self._h, img.data_ptr(), dt, img.shape[0], plane_set, sp))
        return img.shape[0]

    def fold(self, batch: int, plane_set: int, buf: int, stream=None):
        """folded GEMM of a time step: plane set -> partial buffer `buf` (ita_vitlstm_fold)"""
        sp = _stream_ptr(self.device) if stream is None else C.c_void_p(stream.cuda_stream)
        _chk(lib().ita_vitlstm_fold(self._h, batch, plane_set, buf, sp))

    def pipelined(self, imgs, desvels, quats, state, vels, stream_front, stream_back):
        """n time steps pipelined on two torch streams by the library (ita_vitlstm_pipelined): imgs / desvels / quats /
        vels are sequences of per-step tensors (or a tensor with a leading step axis), state = (h, c) updated in place"""
        torch = _torch()
        n = len(imgs)
        if n < 1 or not (len(desvels) == len(quats) == len(vels) == n):
            raise ITAError("pipelined: imgs / desvels / quats / vels must hold one tensor per step")
        checked = [self._image(im) for im in imgs]       # device ordinal, (60, 90), dtype, contiguity -- as forward does
        if len({dt for _, dt in checked}) != 1 or len({im.shape[0] for im, _ in checked}) != 1:
            raise ITAError("pipelined: every step must have the same batch and image dtype")
        imgs, dt = [im for im, _ in checked], checked[0][1]
        B = imgs[0].shape[0]

        def same(ts, shape, what):
            out = []
            for t in ts:
                if not t.is_cuda or t.device.index != self.device or t.dtype != torch.float32 or not t.is_contiguous() \
                        or t.numel() != int(np_prod(shape)):
                    raise ITAError(f"pipelined: every {what} must be a contiguous f32 tensor of {shape} on cuda:{self.device}")
                out.append(t)
            return out
        desvels, quats, vels = same(desvels, (B,), "desvel"), same(quats, (B, 4), "quat"), same(vels, (B, 3), "vel")
        same(state, (3, B, 128), "state tensor")
        arr = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])
        _chk(lib().ita_vitlstm_pipelined(self._h, arr(imgs), dt, arr(desvels), arr(quats), state[0].data_ptr(), state[1].data_ptr(),
                                         arr(vels), B, n, C.c_void_p(stream_front.cuda_stream), C.c_void_p(stream_back.cuda_stream)))

    def back(self, desvel, quat, hidden, out, buf: int, stream=None):
        """state half of a time step (LSTM + fc) from buffer `buf`; out = (vel, h_out, c_out) tensors"""
        B = out[0].shape[0]
        sp = _stream_ptr(self.device) if stream is None else C.c_void_p(stream.cuda_stream)
        _chk(lib().ita_vitlstm_back(self._h, desvel.data_ptr(), quat.data_ptr(), hidden[0].data_ptr(),
                                    hidden[1].data_ptr(), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), B,
                                    buf, sp))

    def forward_slots(self, img, desvel, quat, state_h, state_c, slot_idx):
        """Serving form: state_h/state_c (3, num_slots, 128) persistent, updated in place for the
        streams named by slot_idx (int32 device tensor, distinct).  Returns vel (B,3)."""
        torch = _torch()
        img, dt = self._image(img)
        B = img.shape[0]
        desvel, quat = _dev_f32(desvel).reshape(B), _dev_f32(quat, (B, 4))
        assert state_h.is_contiguous() and state_c.is_contiguous() and state_h.dtype == torch.float32
        slot_idx = slot_idx.to(torch.int32).contiguous()
        vel = torch.empty((B, 3), dtype=torch.float32, device=img.device)
        _chk(lib().ita_vitlstm_forward_slots(self._h, img.data_ptr(), dt, desvel.data_ptr(), quat.data_ptr(),
                                             state_h.data_ptr(), state_c.data_ptr(), slot_idx.data_ptr(),
                                             state_h.shape[1], vel.data_ptr(), B, _stream_ptr(self.device)))
        return vel

    def graphed_step(self, batch: int) -> "GraphedStep":
        """a HIP-graph replay of one time step with static buffers (see GraphedStep)"""
        self.reserve(batch)
        g = GraphedStep(self, batch)
        self._track_graph(g)
        return g

    def pipelined_steps(self, batch: int, n_steps: int = 8, stages: int = 3) -> "PipelinedSteps":
        """n_steps time steps per HIP-graph replay: encoder(t+2) | folded GEMM(t+1) | LSTM + fc(t) on three streams
        (stages = 2: front(t+1) | back(t) on two); see PipelinedSteps"""
        if n_steps < 2 or stages not in (2, 3):
            raise ITAError("pipelined_steps: n_steps >= 2 and stages in (2, 3)")
        self.reserve(batch)
        g = PipelinedSteps(self, batch, n_steps, stages)
        self._track_graph(g)
        return g

    # ---- drop-in symbols (host buffers) --------------------------------------------------
    def bind_dispatch(self, layer: int = 0, dtype: int = DISPATCH_F16):
        _chk(lib().ita_bind_dispatch(self._h, layer, dtype))


class GraphedStep:
    """One time step of ita_vitlstm_forward captured in a HIP graph: at small batch the six kernel launches
    are launch-bound, a graph replays them with one host call.  Static buffers: write `img` (B,60,90) u8,
    `desvel` (B,), `quat` (B,4), then call the object; `vel` (B,3) holds the result, the LSTM state `h`, `c`
    (3,B,128) is updated in place from step to step (zero it to start a new stream)."""

    def __init__(self, engine: "Engine", batch: int):
        torch = _torch()
        dev = torch.device("cuda", engine.device)
        self.engine, self.B = engine, batch
        self.img = torch.zeros((batch, 60, 90), dtype=torch.uint8, device=dev)
        self.desvel = torch.zeros((batch,), dtype=torch.float32, device=dev)
        self.quat = torch.zeros((batch, 4), dtype=torch.float32, device=dev)
        self.quat[:, 0] = 1
        self.h = torch.zeros((3, batch, 128), dtype=torch.float32, device=dev)
        self.c = torch.zeros((3, batch, 128), dtype=torch.float32, device=dev)
        self.vel = torch.zeros((batch, 3), dtype=torch.float32, device=dev)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):          # warm-up outside the capture: workspace, kernel attributes
            for _ in range(2):
                self._step()
        torch.cuda.current_stream(dev).wait_stream(side)
        self.h.zero_()
        self.c.zero_()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self._step()
        self.h.zero_()
        self.c.zero_()

    def _step(self):
        self.engine.forward(self.img, self.desvel, self.quat, (self.h, self.c), out=(self.vel, self.h, self.c))

    def __call__(self):
        self.graph.replay()
        return self.vel


PART_BUFFERS = 8    # ITA_PART_BUFFERS of include/ita_mi355x.h: partial-sum buffers of the front/back form


class PipelinedSteps:
    """`n_steps` consecutive time steps captured in ONE HIP graph.  stages = 3 (default), three streams: the encoder of step
    t+2 (ita_vitlstm_encode), the folded GEMM of step t+1 (ita_vitlstm_fold) and the LSTM layers + fc of step t
    (ita_vitlstm_back) run side by side, with two sets of encoder-output planes and three partial-sum buffers; measured per
    step (tools/pipeline3_probe.py): 1 frame 31.7 us, 64 frames 36.1, 128 frames 38.2, 256 frames 47.7 -- against 34.0 / 39.7 /
    43.0 / 47.6 for stages = 2, which is the rest of this description.
    stages = 2, two streams: the image-only front of step t+1
    (tokenizer, encoder, folded GEMM: ita_vitlstm_front) runs while the recurrent back of step t (LSTM layers, fc:
    ita_vitlstm_back) is still in flight.  The recurrence is respected -- back(t) follows back(t-1) on its stream and
    front(t) -- and so is the reuse of the partial-sum buffers (front(t) waits for back(t - PART_BUFFERS); with n_steps <=
    PART_BUFFERS the front stream never waits for the back stream inside a replay).  This pays when a GPU
    holds few streams (up to ~256: the strong-scaling regime of BASELINE config 4 on 8 GPUs): the encoder then leaves CUs
    free for the small LSTM kernels, and one graph launch replaces 6 * n_steps kernel launches.  At 1024 streams per GPU
    the encoder owns every CU and nothing overlaps (measured), so bench.py uses this below 256 streams only.
    Static buffers: `img` (n,B,60,90) u8, `desvel` (n,B), `quat` (n,B,4) in; `vel` (n,B,3) out; `h`, `c` (3,B,128) carried
    in place from step to step and from replay to replay (zero them to start new streams)."""

    def __init__(self, engine: "Engine", batch: int, n_steps: int = 8, stages: int = 3):
        torch = _torch()
        dev = torch.device("cuda", engine.device)
        self.engine, self.B, self.n, self.stages = engine, batch, n_steps, stages
        if n_steps < 2 or stages not in (2, 3):
            raise ITAError("PipelinedSteps: n_steps >= 2 and stages in (2, 3)")
        engine.reserve(batch)
        self.img = torch.zeros((n_steps, batch, 60, 90), dtype=torch.uint8, device=dev)
        self.desvel = torch.zeros((n_steps, batch), dtype=torch.float32, device=dev)
        self.quat = torch.zeros((n_steps, batch, 4), dtype=torch.float32, device=dev)
        self.quat[..., 0] = 1
        self.h = torch.zeros((3, batch, 128), dtype=torch.float32, device=dev)
        self.c = torch.zeros((3, batch, 128), dtype=torch.float32, device=dev)
        self.vel = torch.zeros((n_steps, batch, 3), dtype=torch.float32, device=dev)
        warm = torch.cuda.Stream(device=dev)
        warm.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(warm):              # outside the capture: kernel attributes, lazy module loads
            for i in range(2):
                engine.front(self.img[i], i & 1, stream=warm)
                engine.back(self.desvel[i], self.quat[i], (self.h, self.c), (self.vel[i], self.h, self.c), i & 1, stream=warm)
        torch.cuda.current_stream(dev).wait_stream(warm)
        torch.cuda.synchronize(dev)
        self.h.zero_()
        self.c.zero_()
        self.graph = torch.cuda.CUDAGraph()
        s_front, s_back = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
        ev_front = [torch.cuda.Event() for _ in range(n_steps)]
        ev_back = [torch.cuda.Event() for _ in range(n_steps)]
        # Two partial buffers, although the library has PART_BUFFERS: with front(i) waiting for back(i-2) the HIP runtime
        # overlaps the two branches of the replayed graph (41.9 us per 128-frame step for 32.6 us of front and 17.3 us of
        # back); without that edge (8 buffers) it runs them one after the other (52.5 us; tools/pipeline_probe.py).
        nb = 2
        if stages == 3:
            # encoder(i+2) | folded GEMM(i+1) | LSTM + fc(i): three branches, two plane sets, three partial buffers
            s_fold = torch.cuda.Stream(device=dev)
            ev_enc = [torch.cuda.Event() for _ in range(n_steps)]
            ev_planes = [torch.cuda.Event() for _ in range(n_steps)]   # (one event per waiter)
            ev_fork = torch.cuda.Event()
            with torch.cuda.graph(self.graph, stream=s_front):
                # both side streams fork from the ORIGIN stream (a stream that joins the capture through an event of
                # another forked stream crashes hipStreamEndCapture on ROCm 7.0)
                ev_fork.record(s_front)
                s_fold.wait_event(ev_fork)
                s_back.wait_event(ev_fork)
                def cap_encode(i):
                    if i >= 2:
                        s_front.wait_event(ev_planes[i - 2])       # encode(i) overwrites the planes fold(i-2) read
                    if i >= 3:
                        # fold(i) overwrites the partials back(i-3) read (three partial buffers).  The edge goes through
                        # the origin stream -- fold(i) follows encode(i) anyway, and back(i-3) is two steps behind the
                        # encoder in steady state -- because a forked stream that waits for an event downstream of its
                        # own earlier work crashes hipStreamEndCapture on ROCm 7.0
                        s_front.wait_event(ev_back[i - 3])
                    engine.encode(self.img[i], i & 1, stream=s_front)
                    ev_enc[i].record(s_front)

                def cap_fold_back(i):
                    s_fold.wait_event(ev_enc[i])
                    engine.fold(batch, i & 1, i % 3, stream=s_fold)
                    ev_front[i].record(s_fold)
                    ev_planes[i].record(s_fold)
                    s_back.wait_event(ev_front[i])
                    engine.back(self.desvel[i], self.quat[i], (self.h, self.c), (self.vel[i], self.h, self.c), i % 3, stream=s_back)
                    ev_back[i].record(s_back)

                # Node order of the capture: step by step, encode(i) fold(i) back(i).  The dependencies are the same in any
                # order, but ROCm 7.0's graph executor is sensitive to it; no other order measured was faster.
                for i in range(n_steps):
                    cap_encode(i)
                    cap_fold_back(i)
                s_front.wait_stream(s_fold)                         # join
                s_front.wait_stream(s_back)
            self.h.zero_()
            self.c.zero_()
            return
        with torch.cuda.graph(self.graph, stream=s_front):
            for i in range(n_steps):
                if i >= nb:
                    s_front.wait_event(ev_back[i - nb])         # front(i) overwrites the partial buffer back(i-nb) read
                engine.front(self.img[i], i % nb, stream=s_front)
                ev_front[i].record(s_front)
                s_back.wait_event(ev_front[i])                  # (also forks s_back into the capture at i = 0)
                engine.back(self.desvel[i], self.quat[i], (self.h, self.c), (self.vel[i], self.h, self.c), i % nb, stream=s_back)
                ev_back[i].record(s_back)
            s_front.wait_stream(s_back)                          # join
        self.h.zero_()
        self.c.zero_()

    def __call__(self):
        self.graph.replay()
        return self.vel


class FusionTailLarge:
    """The fusion tail (PixelShuffle(2) || Upsample x2 align_corners -> cat -> Conv2d 3x3) on an arbitrary
    token grid -- BASELINE config 5 (reference models/ITA_single_layer_upsample_shuffle/QAT/model.py:116-121,
    layer sizes of models/ITA_upsample_shuffle/model.py:70-79).  conv_w (CO, 5E/4, 3, 3), conv_b (CO,): numpy."""

    def __init__(self, conv_w, conv_b, device: Optional[int] = None):
        import numpy as np
        torch = _torch()
        if not torch.cuda.is_available():
            raise ITAError("no GPU visible: the ITA engine has no CPU path")
        self.device = torch.cuda.current_device() if device is None else int(device)
        self._h = C.c_void_p()
        _chk(lib().ita_create(C.byref(self._h), self.device))
        self.reload(conv_w, conv_b)

    def reload(self, conv_w, conv_b):
        """ita_fusion_tail_load on the same handle: replaces the weights, E and CO included"""
        import numpy as np
        w = np.ascontiguousarray(conv_w, dtype=np.float32)
        b = np.ascontiguousarray(conv_b, dtype=np.float32)
        CO, cin = w.shape[0], w.shape[1]
        E = cin * 4 // 5
        if w.shape[2:] != (3, 3) or E // 4 + E != cin or b.shape != (CO,):
            raise ITAError("conv_w must be (CO, 5E/4, 3, 3) and conv_b (CO,)")
        _chk(lib().ita_fusion_tail_load(self._h, w.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), E, CO))
        self.E, self.CO = E, CO

    def __call__(self, x, tok_h: int, tok_w: int, out=None):
        """x (B, tok_h*tok_w, E) f32 on the GPU -> (B, CO, 2 tok_h, 2 tok_w) f32"""
        torch = _torch()
        x = _dev_f32(x)
        B = x.shape[0]
        if x.shape[1] != tok_h * tok_w or x.shape[2] != self.E:
            raise ITAError(f"x must be (B, {tok_h * tok_w}, {self.E})")
        if out is None:
            out = torch.empty((B, self.CO, 2 * tok_h, 2 * tok_w), dtype=torch.float32, device=x.device)
        _chk(lib().ita_fusion_tail_large(self._h, x.data_ptr(), out.data_ptr(), B, tok_h, tok_w, _stream_ptr(self.device)))
        return out

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            lib().ita_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ITAViTLSTM:
    """Mirror of the reference's ``ITALSTMNetVIT_QAT`` call convention (QAT/model.py:93-132)."""

    def __init__(self, blob: bytes, device: Optional[int] = None, reserve: int = 0):
        self.engine = Engine(blob, device, reserve)

    def __call__(self, X: Sequence):
        return self.forward(X)

    def forward(self, X: Sequence):
        img, desvel = X[0], X[1]
        quat = X[2] if len(X) > 2 else None
        hidden = X[3] if len(X) > 3 else None
        return self.engine.forward(img, desvel, quat, hidden)
