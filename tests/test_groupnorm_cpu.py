"""CPU: the GroupNorm offset-class cases (tests/groupnorm_cases.py) are what they claim to be, the float32 restatement sits inside the
bounds the GPU tests set (tests/test_hip_groupnorm.py), a variance by E[y^2] - mean^2 in the summation orders the kernels had does NOT,
and the centred orders the kernels have now do.  The table these tests print is the CPU half of profiles/groupnorm_parity.txt."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import groupnorm_cases as gc

# the emulations walk rows one by one: the 514-block case is left to the device
EMULATED = [s for s in gc.SHAPES if s[1] <= 4161]
_ids = lambda s: "x".join(str(v) for v in s)


@pytest.mark.parametrize("shape", gc.SHAPES, ids=_ids)
def test_exact_family_is_exact_and_on_its_classes(shape):
    case = gc.exact_case(shape)
    st = gc.study(case)
    assert torch.equal(st.y64.float().double(), st.y64)                       # y is exact in fp32 ...
    assert torch.equal((st.y64 / gc.QUANT).round(), st.y64 / gc.QUANT) and float(st.y64.abs().max()) < 1024
    assert torch.equal(st.y32.double(), st.y64)                               # ... and an fp32 convolution finds it
    for t in (case.x, case.w):                                                # operands exact in bf16 (8 bits) and f16
        assert torch.equal(t.bfloat16().float(), t) and torch.equal(t.half().float(), t)
    _on_classes(case, st)
    dead = st.y64[:, case.dead * case.cg:(case.dead + 1) * case.cg]
    assert torch.all(dead == gc.DEAD_VALUE)
    want = case.beta.double()[case.dead * case.cg:(case.dead + 1) * case.cg]
    assert torch.equal(st.ref64[:, case.dead * case.cg:(case.dead + 1) * case.cg], want[None, :, None].expand_as(dead))      # the reference returns beta


def _on_classes(case, st):
    r = gc.measured_ratio(case, st.y64)
    for n in range(case.N):
        for g, (cls, sign) in enumerate(gc.signed_classes(n)):
            if g == case.dead:
                continue
            if cls == 0:          # (the exact family's offsets are multiples of 2^-10: that much of a mean may be left)
                yg = st.y64[n, g * case.cg:(g + 1) * case.cg]
                assert abs(float(yg.mean())) <= max(0.2 * float(yg.std(unbiased=False)), gc.QUANT), (n, g, float(r[n, g]))
            else:
                assert 0.8 * cls <= sign * float(r[n, g]) <= 1.2 * cls, (n, g, cls, sign, float(r[n, g]))


@pytest.mark.parametrize("shape", gc.SHAPES + [gc.SPLITK_SHAPE], ids=_ids)
def test_drawn_family_is_on_its_classes(shape):
    case = gc.drawn_case(shape)
    _on_classes(case, gc.study(case))


@pytest.mark.parametrize("shape", gc.SHAPES, ids=_ids)
def test_float32_restatement_is_inside_the_exact_bound(shape):
    """True by construction (the bound is 8 x this error)."""
    case = gc.exact_case(shape)
    st = gc.study(case)
    for lab in case.labels():
        assert st.err32[lab] <= gc.bound(case, st, lab) / (gc.FACTOR if lab != gc.DEAD else 1.0)
    print("\n" + "\n".join(gc.report("float32 restatement", case, st.err32, st)))


@pytest.mark.parametrize("shape", gc.SHAPES + [gc.SPLITK_SHAPE], ids=_ids)
def test_float32_restatement_on_the_drawn_family(shape):
    """The drawn family's bound is test_conv1x1_groupnorm_unit's 2e-5, per class and relative to the class's scale.  The float32 restatement (an fp32
    convolution in front of an fp32 group_norm) carries the rounding of the mean itself, r 2^-24 and a little more from the convolution's sum: it is under
    2e-5 / 8 up to class 10, 2 - 6e-6 at class 30, 0.7 - 2e-5 at class 100 and 2 - 4.5e-5 at class 300 on these cases.  So the top class, where fp32
    arithmetic as such does not keep 2e-5, is not asserted on the device (drawn_classes_asserted: never more than the top class); every class that is
    asserted there has the restatement inside the bound here."""
    case = gc.drawn_case(shape)
    st = gc.study(case)
    rel = {lab: st.err32[lab] / st.scale[lab] for lab in case.labels()}
    print("\n" + "\n".join(f"float32 restatement (drawn)  {case.name:<26} class {lab:>4}  rel err {rel[lab]:.3e}" for lab in case.labels()))
    asserted = gc.drawn_classes_asserted(case)
    assert set(case.labels()) - set(asserted) <= {gc.CLASSES[-1]}
    for lab in asserted:
        assert rel[lab] < (gc.DRAWN_TOL / gc.FACTOR if lab <= 10 else gc.DRAWN_TOL), (lab, rel[lab])


@pytest.mark.parametrize("shape", EMULATED, ids=_ids)
def test_raw_second_moment_misses_the_bound_and_the_centred_orders_keep_it(shape):
    """Why tests/test_hip_groupnorm.py exists: in the summation orders the kernels had, fp32 E[y^2] - mean^2 leaves 8 x the float32 restatement from
    class 10 upwards (the table: profiles/groupnorm_parity.txt); the centred orders they have now stay inside on every class."""
    case = gc.exact_case(shape)
    st = gc.study(case)
    orders = {"eval, E[y^2] - mean^2": gc.stats_eval_raw, "train, E[y^2] - mean^2": gc.stats_train_raw,
              "eval, centred": gc.stats_eval_centred, "train, centred": gc.stats_train_centred}
    errs = {k: gc.class_err(case, gc.restate(case, st.y32, f), st.ref64) for k, f in orders.items()}
    print()
    for k, e in errs.items():
        print("\n".join(gc.report(k, case, e, st)))
    for k in ("eval, centred", "train, centred"):
        for lab in case.labels():
            assert errs[k][lab] <= gc.bound(case, st, lab), (k, lab, errs[k][lab], st.err32[lab])
        if case.HW <= gc.EXACT_SUMS_HW:
            assert errs[k][gc.DEAD] == 0.0
    # A raw second moment errs by ~ r^2 2^-24, the restatement by ~ r 2^-24.  The eval order (fp32 to the end) is outside from class 10 upwards, the
    # training tier's (float64 over the channels of a group) from class 30; one pixel of two channels has no sum long enough to cancel before class 100.
    for k in ("eval, E[y^2] - mean^2", "train, E[y^2] - mean^2"):
        bad = [lab for lab in gc.CLASSES if errs[k][lab] > gc.FACTOR * st.err32[lab]]
        first = 100 if case.HW == 1 else 10 if k.startswith("eval") else 30
        assert set(bad) >= {lab for lab in gc.CLASSES if lab >= first}, (k, bad)
