"""Weight/scale blob ("ITAW0001", "ITAW0002" for a float32 FFN, "ITAW0003" for the float graph; include/ita_weights.h)
packer.

Turns the reference's converted int8 blocks (int8 weights, float biases, scales -- what
training/qa_train.py:81-95 saves and tests/export_and_validation_W_B.py:47-62 extracts)
plus the float32 parameters of the non-quantised layers into the packed blob that
``ita_load_weights`` uploads.  All requantisation constants are derived here, in the
float32 arithmetic the reference's kernels use (pinned against tests/golden):

* ``nnq.Linear``:  bias_q = rne(b * (1f / f32(f32(s_w) * s_x)));  mult = f32(f32(s_w)*f32(s_x)) / f32(s_out)
* ``matmul1``:     mult = f32(f32(s_q)*f32(s_k)) / f32(s_logit)
* ``matmul2``:     mult = f32((1/255 * s_v) / s_ctx)   (python-double product, tests/export_and_validation_W_B.py:140)
* ``Quantize``:    q = rne(x * (1f / f32(s)))
"""
from __future__ import annotations

import struct
from typing import Dict

import numpy as np

f32 = np.float32
MAGIC = b"ITAW0001"
MAGIC_FFN_F32 = b"ITAW0002"   # the attention-only QAT graph: int8 attention, float32 FFN (ffn%d.w1f / b1f / w2f / b2f)
MAGIC_F32 = b"ITAW0003"       # the float graph: float32 attention (attn%d.wqf ... bof) and float32 FFN
_DT = {np.dtype(np.float32): 0, np.dtype(np.int8): 1, np.dtype(np.int32): 2, np.dtype(np.uint8): 3,
       np.dtype(np.float16): 4}
A_NSCAL, F_NSCAL = 8, 4


def _bias_q(bias, s_w, s_x):
    bsc = f32(float(f32(s_w)) * float(s_x))          # double product of (float w_scale, double in_scale) -> float
    return np.rint(bias.astype(np.float32) * (f32(1.0) / bsc)).astype(np.int32)


def _lin_mult(s_w, s_x, s_out):
    return f32(f32(f32(s_w) * f32(s_x)) / f32(s_out))


def attention_tensors(rec: dict, prefix: str, i: int) -> Dict[str, np.ndarray]:
    """rec: fixture-style record holding '<prefix>q_proj.w_q', '.w_scale', '.bias', '.out_scale', ..."""
    g = lambda k: rec[prefix + k]
    s_x = float(g("quant.scale"))
    s_q, s_k, s_v = (float(g(f"{n}.out_scale")) for n in ("q_proj", "k_proj", "v_proj"))
    s_l, s_c, s_o = float(g("matmul1.scale")), float(g("matmul2.scale")), float(g("out_proj.out_scale"))
    t = {}
    for nm, key, s_in in (("q_proj", "q", s_x), ("k_proj", "k", s_x), ("v_proj", "v", s_x), ("out_proj", "o", s_c)):
        t[f"attn{i}.w{key}"] = np.ascontiguousarray(g(nm + ".w_q").astype(np.int8))
        t[f"attn{i}.b{key}"] = _bias_q(g(nm + ".bias"), g(nm + ".w_scale"), s_in)
    scal = np.zeros(A_NSCAL, np.float32)
    scal[0] = f32(1.0) / f32(s_x)
    scal[1] = _lin_mult(g("q_proj.w_scale"), s_x, s_q)
    scal[2] = _lin_mult(g("k_proj.w_scale"), s_x, s_k)
    scal[3] = _lin_mult(g("v_proj.w_scale"), s_x, s_v)
    scal[4] = f32(f32(f32(s_q) * f32(s_k)) / f32(s_l))
    scal[5] = f32(((1.0 / 255.0) * s_v) / s_c)
    scal[6] = _lin_mult(g("out_proj.w_scale"), s_c, s_o)
    scal[7] = f32(s_o)
    t[f"attn{i}.scal"] = scal
    return t


def ffn_tensors(rec: dict, prefix: str, i: int) -> Dict[str, np.ndarray]:
    g = lambda k: rec[prefix + k]
    s_x, s_1, s_2 = float(g("quant.scale")), float(g("fc1.out_scale")), float(g("fc2.out_scale"))
    t = {f"ffn{i}.w1": np.ascontiguousarray(g("fc1.w_q").astype(np.int8)),
         f"ffn{i}.b1": _bias_q(g("fc1.bias"), g("fc1.w_scale"), s_x),
         f"ffn{i}.w2": np.ascontiguousarray(g("fc2.w_q").astype(np.int8)),
         f"ffn{i}.b2": _bias_q(g("fc2.bias"), g("fc2.w_scale"), s_1)}
    scal = np.zeros(F_NSCAL, np.float32)
    scal[0] = f32(1.0) / f32(s_x)
    scal[1] = _lin_mult(g("fc1.w_scale"), s_x, s_1)
    scal[2] = _lin_mult(g("fc2.w_scale"), s_1, s_2)
    scal[3] = f32(s_2)
    t[f"ffn{i}.scal"] = scal
    return t


def float_tensors(fp: dict, num_layers: int = 1) -> Dict[str, np.ndarray]:
    """float32 layers, keyed by the reference's state_dict names -> blob names."""
    E = fp["tokenizer.conv.weight"].shape[0]
    t = {"tok.conv_w": fp["tokenizer.conv.weight"].reshape(E, 49), "tok.conv_b": fp["tokenizer.conv.bias"],
         "tok.ln_w": fp["tokenizer.norm.weight"], "tok.ln_b": fp["tokenizer.norm.bias"]}
    for i in range(num_layers):
        t[f"norm1_{i}.w"], t[f"norm1_{i}.b"] = fp[f"norms1.{i}.weight"], fp[f"norms1.{i}.bias"]
        t[f"norm2_{i}.w"], t[f"norm2_{i}.b"] = fp[f"norms2.{i}.weight"], fp[f"norms2.{i}.bias"]
        if f"ffn_blocks.{i}.fc1.weight" in fp:   # float FFN (QAT_only_attn): [out][in] as nn.Linear stores it
            f = f"ffn_blocks.{i}."
            t[f"ffn{i}.w1f"], t[f"ffn{i}.b1f"] = fp[f + "fc1.weight"], fp[f + "fc1.bias"]
            t[f"ffn{i}.w2f"], t[f"ffn{i}.b2f"] = fp[f + "fc2.weight"], fp[f + "fc2.bias"]
    if "down_sample.weight" in fp:
        t["tail.conv_w"], t["tail.conv_b"] = fp["down_sample.weight"], fp["down_sample.bias"]
    if "decoder.weight" in fp:
        t["dec.w"], t["dec.b"] = fp["decoder.weight"], fp["decoder.bias"]
        for l in range(3):
            t[f"lstm.w_ih{l}"], t[f"lstm.w_hh{l}"] = fp[f"lstm.weight_ih_l{l}"], fp[f"lstm.weight_hh_l{l}"]
            t[f"lstm.b_ih{l}"], t[f"lstm.b_hh{l}"] = fp[f"lstm.bias_ih_l{l}"], fp[f"lstm.bias_hh_l{l}"]
        t["fc.w"], t["fc.b"] = fp["nn_fc2.weight"], fp["nn_fc2.bias"]
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in t.items()}


def pack_blob(tensors: Dict[str, np.ndarray], E: int, S: int = 128, P: int = 192, F: int = 256, H: int = 1,
              num_layers: int = 1, has_tail: bool = True, ffn_f32: bool = False, attn_f32: bool = False) -> bytes:
    """attn_f32: an ITAW0003 blob (float attention and float FFN); else ffn_f32: ITAW0002; else ITAW0001"""
    names = list(tensors)
    n = len(names)
    hdr_sz, ent_sz = 8 + 4 * 14, 32 + 4 * 6 + 8 * 2
    off = hdr_sz + n * ent_sz
    entries, chunks = [], []
    for nm in names:
        a = np.ascontiguousarray(tensors[nm])
        assert a.dtype in _DT, (nm, a.dtype)
        assert a.ndim <= 4 and len(nm) < 32
        pad = (-off) % 64
        chunks.append(b"\0" * pad)
        off += pad
        shape = list(a.shape) + [0] * (4 - a.ndim)
        entries.append(struct.pack("<32sii4iqq", nm.encode(), _DT[a.dtype], a.ndim, *shape, off, a.nbytes))
        chunks.append(a.tobytes())
        off += a.nbytes
    magic = MAGIC_F32 if attn_f32 else MAGIC_FFN_F32 if ffn_f32 else MAGIC
    hdr = struct.pack("<8s14i", magic, n, E, S, P, F, H, num_layers, int(has_tail), 0, 0, 0, 0, 0, 0)
    assert len(hdr) == hdr_sz and all(len(e) == ent_sz for e in entries)
    return hdr + b"".join(entries) + b"".join(chunks)


def blob_from_record(rec: dict, float_params: dict | None, E: int, num_layers: int = 1, H: int = 1) -> bytes:
    """A record without the int8 FFN (no ``ffn0.fc1.w_q``) is the attention-only graph: its FFN comes from
    float_params (``ffn_blocks.{i}.fc1.weight`` ...) and the blob is an ITAW0002 one.  H: the attention's head count
    (the tensors do not depend on it; the engine runs H in {1, 2, 3, 4, 6} of an ITAW0001 blob)."""
    ffn_f32 = "ffn0.fc1.w_q" not in rec
    if ffn_f32 and (float_params is None or "ffn_blocks.0.fc1.weight" not in float_params):
        raise KeyError("the record has no int8 FFN and float_params no ffn_blocks.{i}.fc1.weight")
    t: Dict[str, np.ndarray] = {}
    for i in range(num_layers):
        t.update(attention_tensors(rec, f"attn{i}.", i))
        if not ffn_f32:
            t.update(ffn_tensors(rec, f"ffn{i}.", i))
    has_tail = False
    if float_params is not None:
        ft = float_tensors(float_params, num_layers)
        if not ffn_f32:   # an int8-FFN blob stays byte-identical whatever else float_params holds
            ft = {k: v for k, v in ft.items() if not (k.startswith("ffn") and k[-1] == "f")}
        t.update(ft)
        has_tail = "tail.conv_w" in t     # without it the decoder reads the flattened tokens (models/ITA/QAT/model.py:80-81)
    return pack_blob(t, E=E, H=H, num_layers=num_layers, has_tail=has_tail, ffn_f32=ffn_f32)


def float_attention_tensors(fp: dict, i: int) -> Dict[str, np.ndarray]:
    """layer i's float attention (models/ITA/layers.py:47-88), [out][in] as nn.Linear stores it -> attn%d.wqf ... bof"""
    a = f"attention_blocks.{i}."
    t = {}
    for nm, key in (("q_proj", "q"), ("k_proj", "k"), ("v_proj", "v"), ("out_proj", "o")):
        t[f"attn{i}.w{key}f"], t[f"attn{i}.b{key}f"] = fp[a + nm + ".weight"], fp[a + nm + ".bias"]
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in t.items()}


def blob_from_float_params(fp: dict, num_layers: int = 1) -> bytes:
    """The float graph (models/ITA_single_layer_upsample_shuffle/model.py:35-140, nothing quantised) -> an ITAW0003 blob.
    fp: every parameter under the reference's state_dict names, spectral norm folded (synth.float_params, or
    float_params_from_state_dict of a float checkpoint)."""
    for i in range(num_layers):
        for k in (f"attention_blocks.{i}.q_proj.weight", f"ffn_blocks.{i}.fc1.weight"):
            if k not in fp:
                raise KeyError(f"float parameters lack {k}")
    t: Dict[str, np.ndarray] = {}
    for i in range(num_layers):
        t.update(float_attention_tensors(fp, i))
    t.update(float_tensors(fp, num_layers))
    E = int(fp["tokenizer.conv.weight"].shape[0])
    P, F = (int(fp[f"{n}.0.{m}.weight"].shape[0]) for n, m in (("attention_blocks", "q_proj"), ("ffn_blocks", "fc1")))
    return pack_blob(t, E=E, P=P, F=F, num_layers=num_layers, has_tail="tail.conv_w" in t, ffn_f32=True, attn_f32=True)


def load_fixture(path: str) -> dict:
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


# ---------------------------------------------------------------------------------------------
# Row n4: from a reference checkpoint to the blob.
#
# training/qa_train.py:81-95 saves ``state_dict()`` of the CONVERTED model
# (model_quantized_final.pth): quantized Linear layers appear as
# ``<name>._packed_params._packed_params = (qint8 weight, float bias)`` plus ``<name>.scale``;
# QuantStubs as ``<block>.quant.scale``; QFunctional matmuls as ``<block>.matmulN.scale``.
# tests/export_and_validation_W_B.py:47-62,233-245 extracts the same items through module hooks;
# here they are read straight from the state_dict, so no reference code is needed.

def _float_ffn(sd: dict, i: int) -> bool:
    """layer i's FFN is a float nn.Linear pair (QAT_only_attn's ITAFeedForward), not a converted int8 one"""
    f = f"ffn_blocks.{i}.fc1."
    return f + "weight" in sd and f + "_packed_params._packed_params" not in sd


def _float_attn(sd: dict, i: int) -> bool:
    """layer i's attention is the float ITASelfAttention (a float checkpoint), not a converted int8 one"""
    a = f"attention_blocks.{i}.q_proj."
    return a + "weight" in sd and a + "_packed_params._packed_params" not in sd


def record_from_state_dict(sd: dict, num_layers: int = 1) -> dict:
    """converted-model state_dict -> the fixture-style record consumed by blob_from_record"""
    def packed(name):
        w, b = sd[name + "._packed_params._packed_params"]
        if int(w.q_zero_point()) != 0:
            raise ValueError(f"{name}: weights must be symmetric (zero_point 0)")
        return w.int_repr().numpy().astype(np.int8), float(w.q_scale()), b.detach().numpy().astype(np.float32)

    def scalar(name):
        return float(np.asarray(sd[name].detach().cpu().numpy()).reshape(-1)[0])

    rec = {}
    for i in range(num_layers):
        a = f"attention_blocks.{i}."
        for nm in ("q_proj", "k_proj", "v_proj", "out_proj"):
            wq, ws, b = packed(a + nm)
            if int(sd[a + nm + ".zero_point"]) != 0:
                raise ValueError(f"{a + nm}: output zero_point must be 0 (ita_symmetric_qconfig)")
            rec[f"attn{i}.{nm}.w_q"], rec[f"attn{i}.{nm}.w_scale"], rec[f"attn{i}.{nm}.bias"] = wq, ws, b
            rec[f"attn{i}.{nm}.out_scale"] = scalar(a + nm + ".scale")
        rec[f"attn{i}.quant.scale"] = scalar(a + "quant.scale")
        rec[f"attn{i}.matmul1.scale"] = scalar(a + "matmul1.scale")
        rec[f"attn{i}.matmul2.scale"] = scalar(a + "matmul2.scale")
        f = f"ffn_blocks.{i}."
        if _float_ffn(sd, i):   # QAT_only_attn: float_params_from_state_dict carries the FFN
            continue
        for nm in ("fc1", "fc2"):
            wq, ws, b = packed(f + nm)
            rec[f"ffn{i}.{nm}.w_q"], rec[f"ffn{i}.{nm}.w_scale"], rec[f"ffn{i}.{nm}.bias"] = wq, ws, b
            rec[f"ffn{i}.{nm}.out_scale"] = scalar(f + nm + ".scale")
        rec[f"ffn{i}.quant.scale"] = scalar(f + "quant.scale")
    return rec


def fold_spectral_norm(sd: dict, name: str):
    """torch.nn.utils.spectral_norm stores weight_orig / weight_u / weight_v; in eval mode the layer
    uses weight_orig / sigma with sigma = u^T W v (models/ITA_single_layer_upsample_shuffle/model.py:81,84).
    The reference's own strict=False load silently drops these keys; fold them explicitly."""
    if name + ".weight" in sd:
        return np.asarray(sd[name + ".weight"].detach().cpu().numpy(), np.float32)
    w = np.asarray(sd[name + ".weight_orig"].detach().cpu().numpy(), np.float64)
    u = np.asarray(sd[name + ".weight_u"].detach().cpu().numpy(), np.float64)
    v = np.asarray(sd[name + ".weight_v"].detach().cpu().numpy(), np.float64)
    sigma = float(u @ (w.reshape(w.shape[0], -1) @ v))
    return (w / sigma).astype(np.float32)


# The reference's model files name the same layers three ways.  models/ITA_single_layer_upsample_shuffle (and its QAT /
# QAT_only_attn variants): attention_blocks.{i} / ffn_blocks.{i} / norms1.{i} / norms2.{i} -- the names used here.
# models/ITA_upsample_shuffle (and models/ITA): norm1_layers.{i} / norm2_layers.{i}.  models/ITA_single_layer: one layer as
# attention_block / ffn_block / norm1 / norm2.
_LAYER_NAMES = (("norm1_layers.", "norms1."), ("norm2_layers.", "norms2."), ("attention_block.", "attention_blocks.0."),
                ("ffn_block.", "ffn_blocks.0."), ("norm1.", "norms1.0."), ("norm2.", "norms2.0."))


def canonical_state_dict(sd: dict) -> dict:
    """sd with its layer names mapped to attention_blocks.{i} / ffn_blocks.{i} / norms1.{i} / norms2.{i}"""
    def ren(k):
        for a, b in _LAYER_NAMES:
            if k.startswith(a):
                return b + k[len(a):]
        return k
    return {ren(k): v for k, v in sd.items()}


def float_params_from_state_dict(sd: dict, num_layers: int = 1) -> dict:
    """non-quantised layers under the reference's state_dict names (float or converted checkpoint).  The decoder's
    width decides the graph: 4608 reads the fusion tail (down_sample is carried); E * 128 reads the flattened tokens,
    and a down_sample the model file declares but never calls is dropped."""
    sd = canonical_state_dict(sd)
    g = lambda k: np.asarray(sd[k].detach().cpu().numpy(), np.float32)
    fp = {k: g(k) for k in ("tokenizer.conv.weight", "tokenizer.conv.bias", "tokenizer.norm.weight",
                            "tokenizer.norm.bias", "decoder.bias", "nn_fc2.bias")}
    fp["decoder.weight"] = fold_spectral_norm(sd, "decoder")
    fp["nn_fc2.weight"] = fold_spectral_norm(sd, "nn_fc2")
    E, width = fp["tokenizer.conv.weight"].shape[0], fp["decoder.weight"].shape[1]
    if width == 4608:
        fp["down_sample.weight"], fp["down_sample.bias"] = g("down_sample.weight"), g("down_sample.bias")
    elif width != E * 128:
        raise ValueError(f"decoder reads {width} features: neither the fusion tail (4608) nor the tokens (E * 128 = {E * 128})")
    for i in range(num_layers):
        for nm in (f"norms1.{i}", f"norms2.{i}"):
            fp[nm + ".weight"], fp[nm + ".bias"] = g(nm + ".weight"), g(nm + ".bias")
        if _float_ffn(sd, i):   # float FFN (QAT_only_attn, or the float model)
            for nm in ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias"):
                fp[f"ffn_blocks.{i}.{nm}"] = g(f"ffn_blocks.{i}.{nm}")
        if _float_attn(sd, i):  # float attention (the float model)
            for nm in ("q_proj", "k_proj", "v_proj", "out_proj"):
                for w in ("weight", "bias"):
                    fp[f"attention_blocks.{i}.{nm}.{w}"] = g(f"attention_blocks.{i}.{nm}.{w}")
    for l in range(3):
        for nm in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
            fp[f"lstm.{nm}_l{l}"] = g(f"lstm.{nm}_l{l}")
    return fp


def blob_from_state_dict(sd: dict, num_layers: int = 1, H: int = 1) -> bytes:
    """a converted (QAT) checkpoint -> ITAW0001 / ITAW0002; a float checkpoint (training's model_000205.pth: float
    attention_blocks.{i}.q_proj.weight, no _packed_params) -> ITAW0003.  Every model file's layer names are accepted
    (canonical_state_dict).  H: the head count the checkpoint was trained with (a state dict does not hold it)."""
    sd = canonical_state_dict(sd)
    fp = float_params_from_state_dict(sd, num_layers)
    kinds = {_float_attn(sd, i) for i in range(num_layers)}
    if kinds == {True}:
        if H != 1:
            raise ValueError("the float graph (ITAW0003) runs with one head")
        return blob_from_float_params(fp, num_layers)
    if len(kinds) > 1:
        raise ValueError("a checkpoint mixing float and converted attention layers has no blob format")
    E = fp["tokenizer.conv.weight"].shape[0]
    return blob_from_record(record_from_state_dict(sd, num_layers), fp, E=E, num_layers=num_layers, H=H)
