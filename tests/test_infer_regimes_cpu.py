"""CPU: the regimes of tests/infer_regime_cases.py.  Every stored (case, regime) meets its screening conditions as stored and a ladder rung
lower does not; the yardstick (tests/f16_sites.py) passes the bounds the device is held to, in float64 and in float32; those bounds can
tell: each wrong restatement of the softmax in traj_train_regime_cases.WRONG, put into the yardstick's softmax, misses them on the pairs of
the regimes it names (NOT_TOLD lists the pairs on which one does not, and why); and the move of the rounding sites out of
tools/error_budget.py kept them intact.  Conditions on the inputs, not on the code under test: nothing here uses the device."""
import json
import os

import pytest
import torch

import axvs_oracle as orc
import f16_sites as fs
import infer_plan_cases as ipc
import infer_regime_cases as rc

PAIRS = rc.pair_ids()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the kernel form per case and pass that the recorded stages name: (spatial denominator from the rounded P, temporal form)
FORMS = {
    "mq2_ffn_rides": [(True, "fused")] * 2, "mq1_frames_32_48": [(True, "fused")] * 2, "first_on_64_rows": [(True, "fused")] * 2,
    "rows16_merged": [(True, "fused")] * 2, "rows16_ragged": [(True, "fused")] * 2, "rows32_merged_split2": [(True, "fused")] * 2,
    "t9_rows16": [(True, "fused")] * 2, "w_over_128_keys": [(True, "fused"), (False, "fused")], "h_under_8_keys": [(False, "fused"), (True, "fused")],
    "maps_temporal_fused": [(False, "fused")] * 2, "t13_reassoc": [(False, "reassoc")] * 2, "t13_no_reassoc": [(False, "generic")] * 2,
    "generic_c64": [(False, "generic")] * 2, "full_272_keys": [(False, "fused")], "full_576_keys": [(False, "fused")],
    "cc_ln_in_kernel": [(True, "fused")], "cc_ln_own_launch": [(False, "reassoc")],
}

# Pairs whose rung the COVERAGE set, not the logit conditions: one rung lower the logits are as sharp as the regime asks, and the named
# coverage condition fails on every one of the 16 seeds.
RAISED_FOR_COVERAGE = {
    ("full_272_keys", "sharp_s"): "gs = 24: no arg-max in the last key chunk more than 104 above the earlier chunks",
    ("full_576_keys", "sharp_s"): "gs = 24: no arg-max in the last key chunk more than 104 above the earlier chunks",
}

# (wrong, case, regime) on which the wrong softmax stays within the bounds, with the reason: the table of DESIGN 6b claims none of these
ONE_TILE = "no frame has more than 16 keys: the first key tile is the only one, its maximum the right one"
NOT_TOLD = {("first_tile_max", n, "sharp_s"): ONE_TILE for n in ("rows16_merged", "t9_rows16", "h_under_8_keys", "maps_temporal_fused", "t13_reassoc",
                                                                 "t13_no_reassoc", "generic_c64", "cc_ln_in_kernel", "cc_ln_own_launch")}
NOT_TOLD["no_max", "full_272_keys", "sharp_t"] = "the largest temporal |s| is 75: exp does not overflow in fp32 and the quotient is right"


def test_the_table():
    assert set(rc.CASES) <= set(ipc.CASES) and set(FORMS) == set(rc.CASES)
    every = {(n, r) for n in rc.CASES for r in rc.REGIMES}
    assert set(rc.PAIRS) | set(rc.LEFT_OUT) == every and not set(rc.PAIRS) & set(rc.LEFT_OUT)
    assert len(rc.LEFT_OUT) <= 3 and all(any((n, r) in rc.PAIRS for r in rc.REGIMES) for n in rc.CASES)
    for (name, regime), pair in rc.PAIRS.items():
        assert 0 <= pair.offset < rc.SEEDS
        assert set(pair.mult) == {"shift": {"mk", "mt"}, "sharp_s": {"gs"}, "sharp_t": {"gt"}}[regime]
        assert all(v in rc.LADDER[regime] for v in pair.mult.values())
    for name in rc.CASES:
        c = rc.case(name)
        assert c.T > 1 and all(L > 1 for *_, L in rc.passes(name))                 # every case has both softmaxes to sharpen
        assert [("psum" in q.on, form) for q, form in rc.forms(name)] == FORMS[name], name
        if any(k == ("first_tile_max", name, "sharp_s") for k in NOT_TOLD):
            assert all(L <= 16 for *_, L in rc.passes(name))
        assert all(set(fs.SITES) <= q.on for q, _ in rc.forms(name))
    assert [-(-L // 256) for n in rc.CHUNKED for *_, L in rc.passes(n)] == [2, 3]
    assert rc.YARD_FACTOR == 2.0 and rc.YARD_CAP == 5e-2 and rc.TOL_F16 == 1e-3


@pytest.mark.parametrize("name,regime", PAIRS)
def test_stored_pair_meets_its_screening_conditions_and_a_rung_lower_does_not(name, regime):
    pair = rc.PAIRS[name, regime]
    misses, report = rc.screen(name, regime, pair.offset, pair.mult)
    print(rc.tag(name, regime))
    print("\n".join(rc.describe(report)))
    assert not misses, misses
    for lower in rc.rung_below(regime, pair.mult):
        if (name, regime) in RAISED_FOR_COVERAGE:
            misses = [m for o in range(rc.SEEDS) for m in rc.screen(name, regime, o, lower)[0][:1]]
            assert len(misses) == rc.SEEDS, (lower, misses)
        else:
            assert rc.screen(name, regime, pair.offset, lower, logit_only=True)[0], lower
    rc._runs.clear()


@pytest.mark.parametrize("name,regime", PAIRS)
def test_the_yardstick_passes_its_own_bounds(name, regime):
    """the emulation with its right softmax is within the bounds (`missed` does not fail everything), run in float64 -- the yardstick itself,
    which must also lie under YARD_CAP on all its seeds -- and in float32, the kernels' own accumulation type"""
    pair = rc.PAIRS[name, regime]
    y = rc.yardstick(name, regime)
    print(rc.tag(name, regime), {k: f"{v:.3e}" for k, v in y.items()})
    assert max(v for k, v in y.items() if not rc.is_map(k)) <= rc.YARD_CAP
    for dtype in (torch.float64, torch.float32):
        assert not rc.missed(name, regime, rc.emulate(name, pair.offset, regime, pair.mult, dtype=dtype))
    assert not rc.plain_missed(name, regime, rc.emulate(name, pair.offset, None, None, dtype=torch.float32))
    rc._runs.clear()


def wrong_pairs(wrong):
    _, _, regimes, chunked_only = rc.WRONG[wrong]
    return [(n, r) for n, r in PAIRS if r in regimes and (not chunked_only or n in rc.CHUNKED)]


@pytest.mark.parametrize("wrong,name,regime", [(w, n, r) for w in rc.WRONG for n, r in wrong_pairs(w)])
def test_the_bounds_tell_a_wrong_softmax(wrong, name, regime):
    """the yardstick in float32 with its softmax stated wrongly, held to the device's bounds"""
    pair = rc.PAIRS[name, regime]
    got = rc.emulate(name, pair.offset, regime, pair.mult, wrong=wrong, dtype=torch.float32)
    misses = rc.missed(name, regime, got)
    print(f"{wrong} on {name} {regime}: {misses[:3] if misses else 'within the bounds'}")
    assert bool(misses) != ((wrong, name, regime) in NOT_TOLD), misses
    rc._runs.clear()


def test_every_wrong_softmax_is_told_somewhere():
    assert {"no_max", "first_tile_max", "neighbour_row_max", "last_tile_dropped", "chunks_not_rescaled", "dead_slots_as_zero"} == set(rc.WRONG)
    for wrong in rc.WRONG:
        for regime in rc.WRONG[wrong][2]:
            assert any((wrong, n, r) not in NOT_TOLD for n, r in wrong_pairs(wrong) if r == regime), (wrong, regime)


def test_the_moved_sites_reproduce_the_recorded_error_budget():
    """tools/error_budget.py's all-sites figure at its default arguments, from the module the sites moved to (float32, 16 sites, the fused
    form): profiles/r2_error_budget.json within 5 % (the fp32 matrix products' summation order is the host library's)"""
    with open(os.path.join(ROOT, "profiles", "r2_error_budget.json")) as f:
        want = json.load(f)["all_sites_fp16"]
    B, T, C, H, W, F = 1, 4, 256, 32, 32, 1024
    assert f"[B={B},T={T},C={C},H={H},W={W}], d_ffn {F}" in open(os.path.join(ROOT, "profiles", "r2_error_budget.json")).read()
    w = orc.random_weights(orc.axial_layer_param_shapes(C, F), 0)
    src, pos = orc.synthetic_clip(B, T, C, H, W, 0)
    ref = orc.axial_layer(src.double(), pos.double(), w, 8, want_attn=False)[0]
    e = fs.layer(src, pos, w, 8, fs.Q(fs.SITES)).double() - ref
    got = [float(e.abs().max() / ref.abs().max()), float(e.norm() / ref.norm())]
    print(got, want)
    assert got == pytest.approx(want, rel=0.05)
