"""Per-stage profiling (ita_profile_begin_sampled / ita_profile_end) on the MI355X: which forwards are counted and which
stages get a time, in all-stage mode, in single-stage mode, through the front/back form and through its encode / fold
halves.  One-layer E = 64 blob, two frames."""
import numpy as np
import pytest

from conftest import golden_files
from drone_oa_iree_vit_accelerator_amd import host, params, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def setup():
    import torch
    fx = params.load_fixture(golden_files("vitlstm_E64_seed0_B2.npz")[0])
    eng = host.Engine(params.blob_from_record(fx, synth.float_params(0, E=64), E=64), device=0)
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    f32 = fx["in0.img_u8"].astype(np.float32) / np.float32(255.0)
    yield eng, {"u8": cu(fx["in0.img_u8"]), "f32": cu(f32)}, cu(fx["in0.desvel"]), cu(fx["in0.quat"])
    eng.close()


def _end(eng):
    import torch
    torch.cuda.synchronize()
    return eng.profile_end()


def test_all_stages_three_forwards(setup):
    eng, img, dv, qt = setup
    eng.profile_begin(4)
    for _ in range(3):
        eng.forward(img["u8"], dv, qt)
    ms, n = _end(eng)
    assert n == 3
    # u8 frames: the tokenizer runs inside the encoder's launch, so the two stages are judged together
    assert ms["tokenizer"] + ms["mha"] > 0 and ms["tail"] > 0 and ms["lstm_fc"] > 0
    assert all(v >= 0 for v in ms.values())


@pytest.mark.parametrize("kind,stage", [("u8", "mha"), ("u8", "tail"), ("u8", "lstm_fc"), ("f32", "tokenizer")])
def test_single_stage_every_second_forward(setup, kind, stage):
    eng, img, dv, qt = setup
    eng.profile_begin(8, every_n=2, only_stage=stage)
    for _ in range(4):
        eng.forward(img[kind], dv, qt)
    ms, n = _end(eng)
    assert n == 2 and ms[stage] > 0
    assert all(v == 0 for k, v in ms.items() if k != stage)


@pytest.mark.parametrize("stage", ["mha", "tail"])
def test_single_stage_through_front(setup, stage):
    eng, img, _, _ = setup
    eng.profile_begin(8, every_n=2, only_stage=stage)
    for _ in range(4):
        eng.front(img["u8"], 0)
    ms, n = _end(eng)
    assert n == 2 and ms[stage] > 0


def test_encode_fold_halves_count_one_forward(setup):
    """the encode half records neither mark of the folded GEMM's stage, so it takes no part in the count"""
    eng, img, _, _ = setup
    eng.profile_begin(8, only_stage="tail")
    eng.encode(img["u8"], 0)
    eng.fold(2, 0, 0)
    ms, n = _end(eng)
    assert n == 1 and ms["tail"] > 0
