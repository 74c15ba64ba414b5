"""CPU: the per-element reference of the deformable-attention sampling op (tests/msda_cases.py) is right, and its band has teeth.
The float64 reference agrees with orc.msda_core (forward directly, gradients through float64 autograd) and with the stored
reference-generated fixtures; a float32 restatement of the kernel arithmetic stays inside the band on every case family, and each of ten
single mutations of it leaves the band on the families named in CATCHES."""
import pytest
import torch

import axvs_oracle as orc
import msda_cases as mc
from golden_util import MSDA_BWD, MSDA_CORE, load, msda_core_inputs, t

_CACHE = {}


def family(name):
    """the cases of a family with their references, computed once (real_sizes at N = 1 here: the GPU file runs them at N = 4)"""
    if name not in _CACHE:
        cases = mc.real_sizes(N=1) if name == "real_sizes" else mc.FAMILIES[name]()
        _CACHE[name] = [(c, mc.reference(c)) for c in cases]
    return _CACHE[name]


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize("name", list(mc.FAMILIES))
def test_reference_agrees_with_the_oracle_and_its_autograd(name):
    for case, ref in family(name):
        v, loc, a = (x.double().requires_grad_(True) for x in (case.value, case.loc, case.aw))
        out = orc.msda_core(v, case.shapes, loc, a)
        out.backward(case.gout.double())
        assert rel(ref["out"].ref, out.detach()) < 1e-12, case
        assert rel(ref["grad_value"].ref, v.grad) < 1e-12 and rel(ref["grad_attn_weight"].ref, a.grad) < 1e-12, case
        # autograd differentiates the weight of the corner at column 0 also for a sample exactly on x == -1 (weight 0, derivative
        # not 0); the op's strict bound gives such a sample no gradient.  Everywhere else the floor-side derivatives coincide.
        wh = torch.tensor([[w, h] for h, w in case.shapes], dtype=torch.float64).view(1, 1, 1, -1, 1, 2)
        on_bound = ((case.loc.double() * wh - 0.5) == -1).any(-1)
        assert bool((ref["grad_sampling_loc"].ref[on_bound] == 0).all()), case
        keep = (~on_bound)[..., None].expand_as(loc.grad)
        assert rel(ref["grad_sampling_loc"].ref * keep, loc.grad * keep) < 1e-12, case
        if not case.exact:
            assert not bool(on_bound.any())


@pytest.mark.parametrize("name", MSDA_CORE + MSDA_BWD)
def test_reference_agrees_with_the_stored_fixtures(name):
    """g14 (float64 autograd of the reference, stored as float32): every element is the float64 value rounded once, within eps32 of it.
    g7: `out64` is the reference in float64, stored as such; `out` is the reference RUN in float32 (grid_sample), held to the band."""
    z, m = load(name)
    value, loc, aw = msda_core_inputs(m)
    N, Lq = loc.shape[:2]
    bwd = "grad_output" in z.files
    gout = t(z["grad_output"]) if bwd else torch.zeros(N, Lq, value.shape[2] * value.shape[3])
    ref = mc.reference(mc.Case(name, "fixture", m["shapes"], value, loc, aw, gout), backward=bwd)
    got = {"out": t(z["out"]).reshape(N, Lq, -1)}
    if bwd:
        got.update(grad_value=t(z["grad_value"]), grad_sampling_loc=t(z["grad_sampling_loc"]), grad_attn_weight=t(z["grad_attn_weight"]))
    else:
        out64 = t(z["out64"]).reshape(N, Lq, -1)
        assert out64.dtype == torch.float64
        assert bool(((out64 - ref["out"].ref).abs() <= 1e-12 * ref["out"].mag0).all()), name
        err = (got.pop("out").double() - ref["out"].ref).abs()
        assert bool((err <= ref["out"].band()).all()), (name, float((err / ref["out"].band()).max()))
    for k, g in got.items():
        r = ref[k]
        err = (g.double() - r.ref).abs()
        assert bool((err <= mc.EPS32 * r.ref.abs() + 1e-45).all()), (name, k, float((err / r.mag0.clamp_min(1e-300)).max()))


@pytest.mark.parametrize("name", list(mc.FAMILIES))
def test_float32_restatement_is_inside_the_band(name):
    for case, ref in family(name):
        rep = mc.ratios(mc.restatement(case), ref)
        print(mc.report_line(case, rep, "fp32-cpu"))
        assert mc.inside(rep), mc.report_line(case, rep)


@pytest.mark.parametrize("name", list(mc.FAMILIES))
def test_excluded_share_of_the_reference(name):
    for case, ref in family(name):
        share = float(ref["near"].double().mean())
        assert share <= mc.MAX_EXCLUDED, (case, share)
        if case.exact:
            assert share == 0.0


def test_lattice_samples_on_the_strict_bounds_contribute_exactly_zero():
    case, ref = [cr for cr in family("lattice") if cr[0].name == "on_the_strict_bounds_all_zero"][0]
    got = mc.restatement(case)
    for k in mc.TENSORS:
        assert bool((ref[k].ref == 0).all()) and bool((ref[k].mag == 0).all()) and bool((got[k] == 0).all()), k


def test_coordinate_rounding_needs_its_own_term():
    """eps32 (n + 8) mag alone -- the band without (mag - mag0) -- is left by correct float32 arithmetic: one sample per query on an
    85-pixel-wide map, where fp32 rounds loc * W - 0.5 by up to 85 eps32 px and a single product has nothing to hide that behind."""
    g = torch.Generator().manual_seed(7)
    shapes = [(49, 85)]
    case = mc._from_px("one_sample_per_query", "probe", shapes, mc._uniform_px(g, shapes, 1, 2000, 1, 1, 0.0), 1, 8)
    ref = mc.reference(case)
    got = mc.restatement(case)
    with_term, without = mc.ratios(got, ref), mc.ratios(got, ref, coord=False)
    print({k: (round(with_term[k][1], 3), round(without[k][1], 3)) for k in with_term})
    assert mc.inside(with_term)
    assert without["out"][1] > 1.0 and without["grad_attn_weight"][1] > 1.0


# which families must catch which mutation (a mutation no family catches would mean a family is missing)
CATCHES = {
    "x_lt_W_to_le_W_minus_1": ["lattice", "border_bands"],
    "x_gt_minus_1_to_ge_0": ["lattice", "border_bands"],
    "right_corner_needs_W_minus_1": ["lattice", "border_bands", "degenerate_maps"],
    "floor_to_round": ["lattice", "head_dims", "contention"],
    "floor_to_trunc": ["lattice", "border_bands"],
    "grad_loc_scale_H_W_swapped": ["lattice", "border_bands", "weights"],
    "lw_hw_swapped_in_one_corner": ["lattice", "head_dims", "contention"],
    "level_start_off_by_one_row": ["lattice", "degenerate_maps", "real_sizes"],
    "attn_weight_of_neighbour_point": ["lattice", "weights", "head_dims"],
    "d0_store_skipped_for_last_sample": ["lattice", "degenerate_maps", "contention"],
}


def test_every_mutation_is_listed():
    assert set(CATCHES) == set(mc.MUTATIONS)


@pytest.mark.parametrize("mut,name", [(m, f) for m, fs in CATCHES.items() for f in fs])
def test_mutation_leaves_the_band(mut, name):
    caught = []
    for case, ref in family(name):
        rep = mc.ratios(mc.restatement(case, mut), ref)
        if not mc.inside(rep):
            caught.append((case.name, {k: v[1] for k, v in rep.items() if v[1] > 1.0}))
    print(mut, name, caught[:2])
    assert caught, f"{mut}: no case of {name} leaves the band"
