"""The cases of softmax_clamp_common are what they claim, on the definition alone (numpy, and the C oracle at H = 1): the
raw logits in front of the clamp are the wanted integers, the classes of rows that make the clamp matter occur often
enough, and three wrong softmax formulas change probs AND out_q on them, so that tests/test_gpu_softmax_clamp.py cannot
pass by missing what it is about, on the tap-less routes either."""
import numpy as np
import pytest

from drone_oa_iree_vit_accelerator_amd import mha_heads_ref as ref
import softmax_clamp_common as scc

f32 = np.float32
FORM_CASES = [(f, c) for f in scc.FORMS for c in scc.CASES]
MIN_ROWS, MIN_MUTANT_ROWS = 16, 32


@pytest.mark.parametrize("form,case", FORM_CASES)
def test_raw_logits_are_the_wanted_integers(form, case):
    e = scc.expect(form, case)
    _, _, ml = scc.FORMS[form]
    raw = np.rint(e["acc"]["L"].astype(np.float32) * ml).astype(np.int64)
    np.testing.assert_array_equal(raw, e["raw"])
    assert raw.min() < -300 and raw.max() > 180
    lg = e["taps"]["logits"].reshape(raw.shape)
    np.testing.assert_array_equal(lg, np.clip(raw, -128, 127))
    pr = e["taps"]["probs"].reshape(raw.shape)
    # the kernels' formula is the definition on these rows (what the comment in ita_stream_kernel.h derives)
    np.testing.assert_array_equal(scc.probs_from_shift(scc.shift_definition(raw)), pr)
    np.testing.assert_array_equal(scc.probs_from_shift(scc.shift_kernel(raw)), pr)
    if case == "h2":
        np.testing.assert_array_equal(raw[:, 1], -raw[:, 0] + 2 * scc.rows_128()[1][:, :, None])
    # V, ctx and out_q are real: the crafted features are not the only content
    assert len(np.unique(e["taps"]["out_q"].reshape(-1, e["E"]), axis=0)) > 64


@pytest.mark.parametrize("form,case", [(f, c) for f, c in FORM_CASES if c != "h2"])
def test_oracle_equals_the_definition(oracle, form, case):
    """at H = 1 the C oracle, which is pinned against the reference, computes these frames as mha_heads_ref does"""
    e = scc.expect(form, case)
    out, taps = oracle.mha(e["x"], e["t"], taps=True)
    np.testing.assert_array_equal(out, e["out"])
    for k, v in taps.items():
        np.testing.assert_array_equal(v, e["taps"][k], err_msg=k)


@pytest.mark.parametrize("form", list(scc.FORMS))
def test_row_classes_occur(form):
    raw = scc.expect(form, "s128")["raw"][:, 0]
    n = dict(a=int(scc.class_a(raw).sum()), b=int(scc.class_b(raw).sum()), c=int(scc.class_c(raw).sum()))
    for v in (127, 128, -128, -129):
        n[f"d{v}"] = int(scc.class_d(raw, v).sum())
    print(f"{form} S = 128: {raw.shape[0] * raw.shape[1]} query rows, raw logits {raw.min()} .. {raw.max()}, classes {n}, "
          f"{int((raw.max(-1) > 127).sum())} with a maximum above 127")
    assert min(n.values()) >= MIN_ROWS, n
    raw2 = scc.expect(form, "h2")["raw"]
    for h in range(2):
        nh = [int(f(raw2[:, h]).sum()) for f in (scc.class_a, scc.class_b, scc.class_c)]
        print(f"{form} H = 2 head {h}: classes a, b, c on {nh} rows")
        assert min(nh) >= MIN_ROWS, (h, nh)
    for S in scc.LONG_S:
        rawl = scc.expect(form, f"long{S}")["raw"][:, 0]
        nl = dict(a=int(scc.class_a(rawl).sum()), b=int(scc.class_b(rawl).sum()), c=int(scc.class_c(rawl).sum()),
                  e=int(scc.class_e(rawl).sum()))
        dead = int((scc.expect(form, f"long{S}")["taps"]["probs"].max(-1) == 0).sum())
        print(f"{form} S = {S}: classes {nl}, {dead} dead rows")
        assert min(nl.values()) >= MIN_ROWS, (S, nl)
        assert dead >= MIN_ROWS and int(scc.class_e(rawl[1]).sum()) >= MIN_ROWS     # (e) on the frame built for it too


@pytest.mark.parametrize("form", list(scc.FORMS))
def test_wrong_formulas_change_probs_and_out_q(form):
    """a kernel with one of three wrong shifts would differ in probs and in out_q on at least 32 query rows of every case,
    so mha, mha_q8, encoder_layer, mha_long_q8 and mha_long, which return no taps, see it too"""
    for case in scc.CASES:
        e = scc.expect(form, case)
        raw, tp = e["raw"], e["taps"]
        pr = tp["probs"].reshape(raw.shape)
        counts = []
        for wrong in scc.MUTANTS:
            p = scc.probs_from_shift(wrong(raw))
            _, out_q = scc.downstream(p, e)
            rows = (p != pr).any(-1).any(1) & (out_q != tp["out_q"]).any(-1)       # (B, S) query rows
            counts.append(int(rows.sum()))
        print(f"{form} {case}: of {raw.shape[0] * raw.shape[2]} query rows, probs and out_q change on "
              + ", ".join(f"{n} ({w.__name__[6:]})" for n, w in zip(counts, scc.MUTANTS)))
        assert min(counts) >= MIN_MUTANT_ROWS, (case, counts)
