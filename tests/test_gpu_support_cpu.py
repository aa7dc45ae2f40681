"""gpu_support's own logic on device="cpu": the canary buffers notice one byte, refused() fails on each of the three ways a
refusal can go wrong, same_bits compares bits."""
import pytest
import torch

from drone_oa_iree_vit_accelerator_amd import host
from gpu_support import FILL, INVALID, UNSUPPORTED, Canaries, cu, refused, same_bits

OUTPUTS = {"row_max": ((2, 5), torch.int8), "col_mass": ((2, 5), torch.int32), "hist": ((2, 3), torch.int64)}
Failed = pytest.fail.Exception


def _canaries(**kw):
    return Canaries(OUTPUTS, device="cpu", **kw)


def _raise(status):
    raise host.ITAError(f"{status}: refused")


def test_untouched_buffers_pass():
    c = _canaries()
    c.assert_untouched()
    c.assert_untouched(written=("col_mass",))
    for k, v in c.views().items():
        v.zero_()                                   # whole outputs written, nothing behind them
    c.assert_untouched(written=tuple(OUTPUTS))
    assert all(len(c.buf[k]) == c.size[k] + 16 for k in OUTPUTS) and c.size == {"row_max": 10, "col_mass": 40, "hist": 48}
    assert len(_canaries(pad=64).buf["hist"]) == 48 + 64
    assert c.ptr("hist", 4) == c.buf["hist"].data_ptr() + 4 and c.ptrs(("hist",)) == {"hist": c.buf["hist"].data_ptr()}


@pytest.mark.parametrize("at", [0, 15])
def test_a_byte_behind_a_written_output_fails_and_is_named(at):
    c = _canaries()
    c.buf["col_mass"][c.size["col_mass"] + at] = 0
    with pytest.raises(AssertionError, match="col_mass"):
        c.assert_untouched(written=tuple(OUTPUTS))
    c.refill()
    c.assert_untouched()


def test_a_byte_of_an_output_not_written_fails_and_is_named():
    c = _canaries()
    c.buf["hist"][7] = 0x76
    with pytest.raises(AssertionError, match="hist"):
        c.assert_untouched(written=("row_max", "col_mass"))
    c.assert_untouched(written=("hist",))           # as a written output its own bytes are free


def test_views_have_the_dtype_and_shape_and_write_through():
    c = _canaries()
    v = c.views()
    for k, (shape, dtype) in OUTPUTS.items():
        assert v[k].dtype == dtype and tuple(v[k].shape) == shape and v[k].data_ptr() == c.ptr(k)
    assert int(v["col_mass"][0, 0]) == 0x77777777 and int(v["row_max"][1, 4]) == FILL
    v["col_mass"][1, 4] = 0x01020304
    assert c.buf["col_mass"][36:40].tolist() == [4, 3, 2, 1] and bool((c.buf["col_mass"][40:] == FILL).all())
    c.refill()
    assert int(c.views()["col_mass"][1, 4]) == 0x77777777


def test_refused_passes_on_a_clean_refusal():
    refused(lambda: _raise(INVALID), _canaries(), INVALID)


def test_refused_fails_when_the_call_does_not_raise():
    with pytest.raises(Failed):
        refused(lambda: None, _canaries(), INVALID)


def test_refused_fails_on_another_status():
    with pytest.raises(AssertionError):
        refused(lambda: _raise(UNSUPPORTED), _canaries(), INVALID)


def test_refused_fails_when_the_refused_call_wrote_a_byte():
    c = _canaries()

    def call():
        c.views()["row_max"][0, 0] = 0
        _raise(INVALID)
    with pytest.raises(AssertionError, match="row_max"):
        refused(call, c, INVALID)


def test_same_bits():
    a = {"x": torch.tensor([0.0, 1.0]), "n": torch.tensor([1, 2], dtype=torch.int32)}
    assert same_bits(a, {k: v.clone() for k, v in a.items()}, ("x", "n"))
    assert torch.equal(a["x"], torch.tensor([-0.0, 1.0])) and not same_bits(a, {"x": torch.tensor([-0.0, 1.0])}, ("x",))
    nan = {"x": torch.tensor([float("nan")])}
    assert same_bits(nan, {"x": nan["x"].clone()}, ("x",))                       # equal bits, though nan != nan
    assert not same_bits(a, {"n": a["n"].to(torch.int64)}, ("n",))               # equal values, another dtype
    assert not same_bits(a, {"n": a["n"].view(torch.float32)}, ("n",))           # equal bits, another dtype
    assert not same_bits(a, {"x": a["x"].reshape(1, 2)}, ("x",))


def test_cu_copies_read_only_and_strided_arrays():
    import numpy as np
    a = np.arange(12, dtype=np.float32).reshape(3, 4)
    a.setflags(write=False)
    t = cu(a.T, device="cpu")
    assert t.is_contiguous() and tuple(t.shape) == (4, 3) and np.array_equal(t.numpy(), a.T)
    t[0, 0] = 5.0
    assert a[0, 0] == 0.0
    u = cu(np.array([0, 65535], np.uint16), device="cpu")
    assert u.dtype == torch.uint16 and u.view(torch.int16).tolist() == [0, -1]
