"""Trajectory replay harness: PNG frames + data.csv -> velocities + L2 error.

MI355X counterpart of the reference's training-set replay host
(samples/inference_trainingset_custom_dispatch/main.cpp:90-193 main loop, :213-246 load_telemetry_for_image,
:260-292 print_output_tensor).  Same data conventions:

  <root>/<trajectory>/data.csv       header line, then rows with more than 12 comma-separated columns:
                                     [1] timestamp, [2] desired velocity, [3..6] quaternion w,x,y,z,
                                     [10..12] ground-truth velocity x,y,z               (main.cpp:223-240)
  <root>/<trajectory>/<stamp>.png    depth frame; the file stem is its timestamp; matched to the CSV row with
                                     |csv_ts - stamp| < 0.001, first match wins            (main.cpp:216,224-226)
  no matching row                    desired velocity 0, quaternion [1,0,0,0], ground truth 0  (main.cpp:143-149)
  trajectories without data.csv      skipped                                                (main.cpp:109)
  LSTM state                         zero at the start of every trajectory, carried frame to frame (main.cpp:100-106)
  graph inputs                       image / 255, desired velocity / 10 (the graph divides by 10 again), quaternion
                                                                                            (main.cpp:128-133,155)
  error                              Euclidean distance between the raw model output and the ground truth (:282-287)

What differs is the schedule (the default one, "steps"; "sequence" is described at replay()): the reference walks one trajectory after the other, one frame per graph call.
Trajectories are independent streams, so here step t runs frame t of EVERY trajectory that still has frames in
one batched call with slot-indexed state (ita_vitlstm_forward_slots): results per trajectory are the same as
the sequential walk (a frame's result does not depend on its batch -- tests/test_gpu_parity.py), the GPU sees
batches instead of single frames.

Frames that are not 90 x 60, in replay() and with replay_frames(..., resize="pil"): resized on the host with PIL's bilinear filter, after a
conversion to 8 bits.  The reference uses stbir_resize_uint8_linear (stb is vendored there, not part of this path): the
two filters are not bit-identical, so in this mode parity with the reference for resized frames is UNPINNED; 90 x 60
frames go through untouched.

With replay_frames(..., resize="stb") the reference host's resize IS reproduced, and pinned: 8-bit frames (16-bit PNGs
converted to 8 bits first, as stbi_load(..., 1) does) that are not 90 x 60 are uploaded at native size and resized by
Engine.ingest_wire -- stb_image_resize2's default filters, Mitchell down and Catmull-Rom up, edge clamp -- to u8 wire
frames, and every frame runs on the u8 wire path.  How it is pinned: ingest_wire_ref.ingest_wire_reference restates the
filter from its formulas, the kernel equals it bit for bit, and it is held to stb's own output on recorded fixtures
(tests/golden/resize_stb_*.npz): every code within 1 of stb's, a differing code only where the value before truncation
lies within 1e-3 of an integer (stb sums its taps in SIMD order; at most one such code per 5400 was seen).

With replay_frames(..., resize="gpu") such frames are uploaded at their native size and depth -- 8-bit, or 16-bit ("I;16") depth PNGs with
their full codes -- and resized by Engine.ingest, then run on the float32 image path.  That resize is the MODEL's own
(refine_inputs: bilinear, align_corners=False), and it is pinned: ingest_ref.ingest_reference defines it and the kernel
equals it bit for bit.  It is not the reference HOST's stb filter (that is resize="stb").  90 x 60 8-bit
frames stay on the u8 wire path; the other frames of one trajectory must share one size.

The parsing half of this module (scan_root, load_telemetry, read_frame) needs no GPU; replay() does.
"""
import math
import os
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

FRAME_W, FRAME_H = 90, 60          # main.cpp:123-124
TS_EPSILON = 0.001                 # main.cpp:216


@dataclass
class Telemetry:
    desired_velocity: float = 0.0
    quaternion: tuple = (1.0, 0.0, 0.0, 0.0)
    ground_truth_velocity: tuple = (0.0, 0.0, 0.0)
    found: bool = False


@dataclass
class Trajectory:
    name: str
    frames: List[str] = field(default_factory=list)        # sorted PNG paths
    telemetry: List[Telemetry] = field(default_factory=list)


def _stof(s: str) -> float:
    """std::stof / std::stod accept leading blanks and trailing junk; raise ValueError like invalid_argument"""
    s = s.strip()
    try:
        return float(s)
    except ValueError:
        # longest numeric prefix, as strtod would take it
        for n in range(len(s) - 1, 0, -1):
            try:
                return float(s[:n])
            except ValueError:
                continue
        raise


def load_rows(csv_path: str):
    """rows of data.csv after the header, split on ',' exactly like the reference (no quoting rules)"""
    with open(csv_path, "r", newline="") as f:
        lines = f.read().splitlines()
    return [ln.split(",") for ln in lines[1:]]


def load_telemetry(rows, stamp: str) -> Telemetry:
    """main.cpp:213-246 for one image: first row with > 12 columns whose column 1 is within 1 ms of the stamp."""
    try:
        ts = _stof(stamp)
    except ValueError:
        return Telemetry()
    for row in rows:
        if len(row) <= 12:
            continue
        try:
            if abs(_stof(row[1]) - ts) < TS_EPSILON:
                return Telemetry(_stof(row[2]), tuple(_stof(row[i]) for i in (3, 4, 5, 6)),
                                 tuple(_stof(row[i]) for i in (10, 11, 12)), True)
        except ValueError:
            continue                    # the reference swallows invalid_argument and keeps scanning
    return Telemetry()


def scan_root(root: str) -> List[Trajectory]:
    """sorted trajectory directories, each with its sorted *.png and the matched telemetry (main.cpp:90-114)"""
    out = []
    for name in sorted(os.listdir(root)):
        tdir = os.path.join(root, name)
        if not os.path.isdir(tdir):
            continue
        csv_path = os.path.join(tdir, "data.csv")
        if not os.path.exists(csv_path):
            continue
        rows = load_rows(csv_path)
        frames = sorted(os.path.join(tdir, f) for f in os.listdir(tdir) if os.path.splitext(f)[1] == ".png")
        tel = [load_telemetry(rows, os.path.splitext(os.path.basename(p))[0]) for p in frames]
        out.append(Trajectory(name, frames, tel))
    return out


def read_frame(path: str) -> Optional[np.ndarray]:
    """u8 (60, 90) depth frame: first channel semantics of stbi_load(..., 1) = luminance; resized if needed"""
    from PIL import Image
    try:
        with Image.open(path) as im:
            im = im.convert("L")
            if im.size != (FRAME_W, FRAME_H):
                im = im.resize((FRAME_W, FRAME_H), Image.BILINEAR)
            return np.asarray(im, dtype=np.uint8).copy()
    except Exception:
        return None                      # the reference warns and skips the image (main.cpp:121)


def read_frame_native(path: str) -> Optional[np.ndarray]:
    """the frame at the size and depth of its file: uint16 (H, W) for a 16-bit grey PNG, else uint8 (H, W) luminance"""
    from PIL import Image
    try:
        with Image.open(path) as im:
            if im.mode in ("I;16", "I;16L", "I;16B", "I;16N"):
                return np.asarray(im).astype(np.uint16)
            return np.asarray(im.convert("L"), dtype=np.uint8).copy()
    except Exception:
        return None


def read_frame_u8(path: str) -> Optional[np.ndarray]:
    """the frame at the size of its file as 8 bits, the way stbi_load(..., 1) hands it to the reference host: a 16-bit
    grey PNG keeps the high byte of every code, anything else is its luminance"""
    im = read_frame_native(path)
    if im is not None and im.dtype == np.uint16:
        im = (im >> 8).astype(np.uint8)
    return im


def _is_wire(im: np.ndarray) -> bool:
    return im.dtype == np.uint8 and im.shape == (FRAME_H, FRAME_W)


def _check_one_size(traj: "Trajectory", seen: dict, key, im: np.ndarray):
    """resize="gpu": the frames of a trajectory that are not u8 90 x 60 share one size"""
    if _is_wire(im):
        return
    if seen.setdefault(key, im.shape) != im.shape:
        raise ValueError(f"trajectory {traj.name}: frames of {seen[key][1]} x {seen[key][0]} and of {im.shape[1]} x "
                         f"{im.shape[0]}; with resize='gpu' the frames that are not 90 x 60 must share one size")


def _ingest_frames(engine, frames: List[np.ndarray], dev):
    """host frames of any size / depth -> (n, 60, 90) f32 on the GPU: one Engine.ingest call per (size, dtype)"""
    import torch
    out = torch.empty((len(frames), FRAME_H, FRAME_W), dtype=torch.float32, device=dev)
    groups = {}
    for j, im in enumerate(frames):
        groups.setdefault((im.shape, im.dtype.str), []).append(j)
    for idx in groups.values():
        raw = torch.from_numpy(np.stack([frames[j] for j in idx])).to(dev)
        out[torch.tensor(idx, device=dev)] = engine.ingest(raw)
    return out


def _wire_frames(engine, frames: List[np.ndarray], dev):
    """resize="stb": host u8 frames of any size -> (n, 60, 90) u8 wire frames on the GPU: 90 x 60 frames as they are, the
    others through one Engine.ingest_wire call per size"""
    import torch
    out = torch.empty((len(frames), FRAME_H, FRAME_W), dtype=torch.uint8, device=dev)
    groups = {}
    for j, im in enumerate(frames):
        groups.setdefault(im.shape, []).append(j)
    for shape, idx in groups.items():
        raw = torch.from_numpy(np.stack([frames[j] for j in idx])).to(dev)
        out[torch.tensor(idx, device=dev)] = raw if shape == (FRAME_H, FRAME_W) else engine.ingest_wire(raw)
    return out


@dataclass
class FrameResult:
    trajectory: str
    frame: str
    output: np.ndarray                   # raw model output (3,)
    ground_truth: np.ndarray
    error: float
    telemetry_found: bool


SCHEDULES = ("steps", "sequence")
RESIZES = ("pil", "gpu", "stb")


def _result(traj: Trajectory, k: int, vel: np.ndarray) -> FrameResult:
    tel = traj.telemetry[k]
    gt = np.asarray(tel.ground_truth_velocity, dtype=np.float32)
    d = vel - gt
    err = float(math.sqrt(float(d[0]) * float(d[0]) + float(d[1]) * float(d[1]) + float(d[2]) * float(d[2])))
    return FrameResult(traj.name, os.path.basename(traj.frames[k]), vel.copy(), gt, err, tel.found)


def _sequence_call(engine, dev, streams, hidden=None, to_wire=False):
    """one Engine.forward_sequence call: streams = per stream [(Telemetry, frame)], the frames of the call either all u8
    90 x 60 (the u8 wire path) or none of them (Engine.ingest, the float32 path), or with to_wire u8 frames of any size
    (Engine.ingest_wire, the u8 wire path) -> (vel (T,B,3) numpy, (h, c))"""
    import torch
    T, B = max(len(q) for q in streams), len(streams)
    native = to_wire or not _is_wire(next(im for q in streams for _, im in q))
    imgs = None if native else np.zeros((T, B, FRAME_H, FRAME_W), np.uint8)
    cells, raws = [], []                             # native: flat (step * B + b) cell of every frame handed to ingest
    dv = np.zeros((T, B), np.float32)
    qt = np.zeros((T, B, 4), np.float32)
    qt[..., 0] = 1.0
    for b, q in enumerate(streams):
        for step, (tel, im) in enumerate(q):
            if native:
                cells.append(step * B + b)
                raws.append(im)
            else:
                imgs[step, b] = im
            # the same float32 values the step schedule hands over (a Python float divided, then rounded once)
            dv[step, b] = tel.desired_velocity / 10.0
            qt[step, b] = tel.quaternion
    lengths = torch.tensor([len(q) for q in streams], dtype=torch.int32, device=dev)
    if native:
        imgs_dev = torch.zeros((T * B, FRAME_H, FRAME_W), dtype=torch.uint8 if to_wire else torch.float32, device=dev)
        imgs_dev[torch.tensor(cells, device=dev)] = (_wire_frames if to_wire else _ingest_frames)(engine, raws, dev)
        imgs_dev = imgs_dev.reshape(T, B, FRAME_H, FRAME_W)
    else:
        imgs_dev = torch.from_numpy(imgs).to(dev)
    vel, hidden = engine.forward_sequence(imgs_dev, torch.from_numpy(dv).to(dev), torch.from_numpy(qt).to(dev), hidden, lengths)
    return vel.cpu().numpy(), hidden


def _replay_sequence(engine, trajs: List[Trajectory], max_batch: int, resize: str = "pil") -> List[FrameResult]:
    """groups of at most max_batch trajectories, each group one Engine.forward_sequence call from zero state: the frames
    of a trajectory are time steps, the trajectories of a group are streams.  resize="gpu": a call takes one image type,
    so a group is cut by what its trajectories hold -- those of u8 90 x 60 frames only run as one call on the u8 wire
    path (as every group does with resize="pil"), those without any such frame as one call through Engine.ingest, and a
    trajectory that mixes the two runs alone, one call per run of consecutive frames of a kind with its state carried
    from call to call (equal to one call: forward_sequence does not depend on how the steps are cut).  A frame's result
    does not depend on the streams beside it, so the cut changes no result.  resize="stb": every frame becomes a u8 wire
    frame (Engine.ingest_wire), so a group is one call again."""
    import torch
    dev = torch.device("cuda", engine.device)
    to_wire = resize == "stb"
    reader = {"pil": read_frame, "gpu": read_frame_native, "stb": read_frame_u8}[resize]
    is_wire = (lambda im: True) if to_wire else _is_wire
    out = []
    for g0 in range(0, len(trajs), max_batch):
        group = trajs[g0:g0 + max_batch]
        seqs = []                                        # per trajectory: [(frame index, frame)] of its readable frames
        for t in group:
            fr = [(k, reader(p)) for k, p in enumerate(t.frames)]
            seqs.append([(k, im) for k, im in fr if im is not None])   # unreadable frames drop out of the sequence
            seen = {}
            for _, im in seqs[-1]:
                if not to_wire:
                    _check_one_size(t, seen, 0, im)
        if max(len(q) for q in seqs) == 0:
            continue
        vels = [None] * len(group)                       # per trajectory: (steps, 3)
        kinds = [{is_wire(im) for _, im in q} for q in seqs]
        for want in ({True}, {False}):                   # an empty trajectory rides with the wire ones, as it always did
            part = [b for b, kd in enumerate(kinds) if kd == want or (not kd and want == {True})]
            if not any(seqs[b] for b in part):
                continue
            vel, _ = _sequence_call(engine, dev, [[(group[b].telemetry[k], im) for k, im in seqs[b]] for b in part],
                                    to_wire=to_wire)
            for j, b in enumerate(part):
                vels[b] = vel[:len(seqs[b]), j]
        for b, kd in enumerate(kinds):
            if len(kd) < 2:
                continue
            hidden, rows, q = None, [], seqs[b]
            start = 0
            for i in range(1, len(q) + 1):               # runs of consecutive frames of one kind
                if i == len(q) or _is_wire(q[i][1]) != _is_wire(q[start][1]):
                    vel, hidden = _sequence_call(engine, dev, [[(group[b].telemetry[k], im) for k, im in q[start:i]]], hidden)
                    rows.append(vel[:, 0])
                    start = i
            vels[b] = np.concatenate(rows)
        for b, (t, q) in enumerate(zip(group, seqs)):
            out.extend(_result(t, k, vels[b][step]) for step, (k, _) in enumerate(q))
    return out


def replay(engine, root: str, max_batch: int = 1024, schedule: str = "steps") -> List[FrameResult]:
    """replay_frames with the host resize (resize="pil"): frames that are not 90 x 60 are resized by PIL as 8 bits.  This
    entry keeps its signature; the choice of the resize is replay_frames' own argument."""
    return replay_frames(engine, root, max_batch, schedule, "pil")


def replay_frames(engine, root: str, max_batch: int = 1024, schedule: str = "steps", resize: str = "pil") -> List[FrameResult]:
    """Runs every trajectory under root through `engine` (host.Engine with a full ITAViTLSTM blob) and returns
    one FrameResult per readable frame, ordered by (trajectory, frame).  Needs a GPU.

    schedule "steps" (default): step t runs frame t of every trajectory that still has frames, one batched call per
    step.  "sequence": every trajectory is handed over whole (Engine.forward_sequence, padded to the longest of its
    group, with lengths), so the encoder sees all frames of a group at once and the recurrence runs inside one kernel
    launch per chunk; the same results bit for bit.  It pays for data sets of a few long trajectories (the step
    schedule then runs at a handful of frames per call).  The GPU part alone, Engine.forward_sequence against a loop of
    Engine.forward on frames already in device memory (tools/bench_sequence.py), takes 0.25 x the time per step at up to 8
    trajectories and 0.43 x at 128, and 12 % MORE at 1024 trajectories per group, which is why "steps" stays the default;
    This function itself also decodes the PNGs on the host and has not been timed.  It holds a whole group's frames in memory
    at once.

    resize "pil" (default): frames that are not 90 x 60 are resized on the host (read_frame).  "gpu": they are uploaded
    at native size and depth (u8, or 16-bit depth PNGs) and resized by Engine.ingest -- the model's own refine_inputs
    resize, pinned by ingest_ref.ingest_reference -- then run as float32 frames; 90 x 60 u8 frames stay on the u8 wire
    path in both schedules ("steps": a call of their own beside the float32 frames of the same step; "sequence": see
    _replay_sequence), so their results are those of replay().  The frames of one
    trajectory that are not 90 x 60 must share one size (ValueError otherwise).  "stb": the reference host's own resize
    -- frames are read as 8 bits at native size (16-bit PNGs converted first), those that are not 90 x 60 resized by
    Engine.ingest_wire (stb's default filters, pinned by ingest_wire_ref.ingest_wire_reference), and ALL frames run as u8
    wire frames: one call per step or per group, any mix of sizes."""
    if schedule not in SCHEDULES:
        raise ValueError(f"schedule must be one of {SCHEDULES}, got {schedule!r}")
    if resize not in RESIZES:
        raise ValueError(f"resize must be one of {RESIZES}, got {resize!r}")
    if resize == "stb" and not callable(getattr(type(engine), "ingest_wire", None)):
        # judged with the other arguments, before the root is read or the engine used: an engine-like object without the
        # wire ingest (a stand-in, an engine of an older build) cannot run this mode, and there is no host fallback for it
        raise ValueError(f"resize='stb' needs an engine with ingest_wire (host.Engine), got {type(engine).__name__}")
    import torch
    trajs = scan_root(root)
    if schedule == "sequence":
        return _replay_sequence(engine, trajs, max_batch, resize) if trajs else []
    reader = {"pil": read_frame, "gpu": read_frame_native, "stb": read_frame_u8}[resize]
    to_wire = resize == "stb"
    seen = {}
    n = len(trajs)
    if n == 0:
        return []
    dev = torch.device("cuda", engine.device)
    state_h = torch.zeros((3, n, 128), device=dev)      # zero = fresh trajectory (main.cpp:100-106)
    state_c = torch.zeros((3, n, 128), device=dev)
    cursor = [0] * n
    results = {i: [] for i in range(n)}
    while True:
        batch = []                                       # (trajectory index, frame index, u8 frame)
        for i, t in enumerate(trajs):
            while cursor[i] < len(t.frames) and len(batch) < max_batch:
                k = cursor[i]
                cursor[i] += 1
                img = reader(t.frames[k])
                if img is not None:                      # unreadable frames are skipped, state untouched
                    if not to_wire:
                        _check_one_size(t, seen, i, img)
                    batch.append((i, k, img))
                    break
        if not batch:
            break
        # the u8 wire frames of the step, then (resize="gpu" only) its native frames through ingest: two calls on
        # disjoint slots, and a frame's result does not depend on the batch it runs in
        # (resize="stb": every frame of the step becomes a u8 wire frame, one call)
        for part in ([b for b in batch if to_wire or _is_wire(b[2])], [b for b in batch if not (to_wire or _is_wire(b[2]))]):
            if not part:
                continue
            if to_wire:
                imgs = _wire_frames(engine, [b[2] for b in part], dev)
            elif _is_wire(part[0][2]):
                imgs = torch.from_numpy(np.stack([b[2] for b in part])).to(dev)
            else:
                imgs = _ingest_frames(engine, [b[2] for b in part], dev)
            tel = [trajs[i].telemetry[k] for i, k, _ in part]
            dv = torch.tensor([t.desired_velocity / 10.0 for t in tel], dtype=torch.float32, device=dev)
            qt = torch.tensor([t.quaternion for t in tel], dtype=torch.float32, device=dev)
            slots = torch.tensor([b[0] for b in part], dtype=torch.int32, device=dev)
            vel = engine.forward_slots(imgs, dv, qt, state_h, state_c, slots).cpu().numpy()
            for j, (i, k, _) in enumerate(part):
                results[i].append(_result(trajs[i], k, vel[j]))
    return [r for i in range(n) for r in results[i]]


def summarize(results: List[FrameResult]) -> dict:
    """per trajectory and overall: frame count, mean and max L2 error"""
    out, by = {}, {}
    for r in results:
        by.setdefault(r.trajectory, []).append(r.error)
    for k, v in by.items():
        out[k] = {"frames": len(v), "mean_error": float(np.mean(v)), "max_error": float(np.max(v))}
    allv = [r.error for r in results]
    out["_all"] = {"frames": len(allv), "mean_error": float(np.mean(allv)) if allv else 0.0,
                   "max_error": float(np.max(allv)) if allv else 0.0}
    return out
