"""The device-side protocol the GPU tests share: uploads, bit comparison, the status strings, canary-filled output
buffers, "a refused call wrote nothing", "one call captured, replayed twice" and the module-scoped engine pool.
cu and Canaries take the device (refused follows its canaries'), so test_gpu_support_cpu.py holds their logic on the CPU."""
import math

import numpy as np
import pytest
import torch

from drone_oa_iree_vit_accelerator_amd import host

INVALID, UNSUPPORTED = "ita status -1", "ita status -4"
FILL = 0x77


def cu(a, device="cuda"):
    """a C-ordered copy of `a` on the device: the cached cases' arrays are read-only; uint16 goes up as the same bits"""
    a = np.array(a, order="C")
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).to(device).view(torch.uint16)
    return torch.from_numpy(a).to(device)


def to_numpy(t):
    return {k: v.cpu().numpy() for k, v in t.items()}


def same_bits(a, b, names):
    """a[k] and b[k] have one dtype, one shape and the same bytes for every k of names: -0.0 is not +0.0"""
    raw = lambda v: v.contiguous().reshape(-1).view(torch.uint8)
    return all(a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and torch.equal(raw(a[k]), raw(b[k])) for k in names)


class Canaries:
    """one byte buffer of 0x77 per output {name: (shape, torch dtype)}, `pad` bytes longer than the output: what a call
    must not write is the pad behind an output it was given and every byte of one it was not"""

    def __init__(self, outputs, pad=16, device="cuda"):
        self.outputs = {k: (tuple(int(n) for n in shape), dtype) for k, (shape, dtype) in outputs.items()}
        self.size = {k: math.prod(shape) * torch.empty((), dtype=dtype).element_size() for k, (shape, dtype) in self.outputs.items()}
        self.buf = {k: torch.full((n + pad,), FILL, dtype=torch.uint8, device=device) for k, n in self.size.items()}

    def ptr(self, name, skew=0):
        return self.buf[name].data_ptr() + skew

    def ptrs(self, names=None):
        return {k: self.ptr(k) for k in (self.buf if names is None else names)}

    def views(self):
        return {k: self.buf[k][:self.size[k]].view(dtype).reshape(shape) for k, (shape, dtype) in self.outputs.items()}

    def refill(self):
        for v in self.buf.values():
            v.fill_(FILL)

    def assert_untouched(self, written=()):
        for k, v in self.buf.items():
            if k in written:
                assert bool((v[self.size[k]:] == FILL).all()), f"bytes behind the output {k} were written"
            else:
                assert bool((v == FILL).all()), f"{k} was written: an output not asked for, or one of a refused call"


def _sync(canaries):
    if next(iter(canaries.buf.values())).is_cuda:
        torch.cuda.synchronize()


def refused(call, canaries, status):
    """call() must raise ITAError with `status` and leave every canary buffer untouched"""
    with pytest.raises(host.ITAError, match=status):
        call()
    _sync(canaries)
    canaries.assert_untouched()


def refused_untouched(eng, fn, x_q, seq_len=None):
    """the int8 entry fn returns ITA_ERR_UNSUPPORTED (-4) before any launch: the sentinel-filled output is untouched"""
    out = torch.full_like(x_q, 77)
    args = (eng._h, 0, x_q.data_ptr(), out.data_ptr(), x_q.shape[0]) + ((seq_len,) if seq_len else ())
    status = fn(*args, host._stream_ptr(eng.device))
    torch.cuda.synchronize()
    return status == -4 and bool((out == 77).all())


def captured_replays(eager, raw_call, canaries, names, replays=2):
    """eager() on a side stream outside the capture (the workspace exists afterwards), raw_call() captured on one stream;
    every replay gives eager()'s bits in the canaries' views of `names` and leaves the rest of the buffers untouched,
    the buffers refilled in between.  Returns eager()'s result."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        want = eager()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        raw_call()
    for replay in range(replays):
        g.replay()
        torch.cuda.synchronize()
        got = canaries.views()
        for k in names:
            assert same_bits(got, want, (k,)), (replay, k)
        canaries.assert_untouched(written=names)
        canaries.refill()
        torch.cuda.synchronize()
    del g
    return want


def engine_pool(blob_of, key_of=lambda *args: args):
    """the generator behind a module's `engines` fixture: get(*args) opens host.Engine(blob_of(*args)) on the first use of
    key_of(*args), all are closed at teardown"""
    made = {}

    def get(*args):
        key = key_of(*args)
        if key not in made:
            made[key] = host.Engine(blob_of(*args), device=0)
        return made[key]
    yield get
    for eng in made.values():
        eng.close()
