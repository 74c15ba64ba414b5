"""GPU: the within-clip training tier at its tier edges and at T up to 16 (tests/traj_train_cases.py: the case table, what each case
reaches in the host code, the measures) -- TemporalAxialTrajectoryAttentionLayer and TemporalTrajectoryAttentionLayer in train() mode,
forward + backward through the C-ABI, against autograd on the float64 oracle.

Per case: out, d_src, d_pos and every parameter gradient under TOL, the gradients that vanish in exact arithmetic under an absolute
noise bound, everything finite, and the ratio r of traj_train_cases (the device's distance from float64 in units of the fp32
oracle's) under R_MARGIN; recompute = True gives the bits of recompute = False; the TWICE cases give the same bits twice.
test_zz_report lists r per case and tensor (profiles/traj_train_parity.txt is that list from an MI355X)."""
import os

import pytest
import torch

import __graft_entry__ as ge
import axvs_oracle as orc
import traj_train_cases as tc

pytestmark = pytest.mark.gpu

TOL = 1e-4
assert tc.TOL == TOL
# r = max|device - f64| / max(max|fp32 oracle - f64|, 2^-24 max|f64|) per case and tensor: out, d_src, d_pos and the parameter gradients
# that do not vanish in exact arithmetic (traj_train_cases.ratios).  Measured on an MI355X over the 21 cases, 592 tensors, every line in
# profiles/traj_train_parity.txt: 0.366 (full_split128, norm2.bias) .. 39.8.  The largest is on the v bias gradient of full_mfma560
# (max|device - f64| 4.7e-4 against the fp32 oracle's 1.2e-5: a column sum over 2240 rows); the
# largest per case is a bias gradient throughout (v, proj_kv, proj, linear1), 17.4 .. 39.8.  The margin is twice the largest, rounded
# up to a power of two (2 * 39.8 = 79.6 -> 128): the factor 2 allows for another summation order at another shape.  TOL stays the hard
# cap whatever r is.  The 47 gradients that vanish in exact arithmetic carry 0 .. 3.5e-7 of the largest gradient norm on the
# device (the largest: axial_l1, height_attn.k.weight) against the bound VANISH_NOISE * R_MARGIN = 1.28e-5.
R_MEASURED = (0.366, 39.8)
R_MARGIN = 128.0
LOG = []
_steps = {}


@pytest.fixture(scope="module", autouse=True)
def built():
    ge.build()
    assert torch.cuda.is_available()


def make_layer(c):
    import axial_vs_amd as ax
    cls = ax.TemporalAxialTrajectoryAttentionLayer if c.kind == "axial" else ax.TemporalTrajectoryAttentionLayer
    layer = cls(c.C, c.F, dropout=c.p_dropout, attn_drop=c.p_attn_drop, n_heads=c.heads)
    layer.load_state_dict(tc.make_weights(c), strict=True)
    layer = layer.cuda().train()
    layer.dropout_seed = tc.dropout_seed(c)
    return layer


def step(name, recompute):
    """one training step of the case on the device -> result dict in the form of traj_train_cases.reference"""
    c = tc.CASES[name]
    src, pos, d_out = tc.make_inputs(c)
    layer = make_layer(c)
    layer.recompute = recompute
    s, p = src.cuda().requires_grad_(True), pos.cuda().requires_grad_(True)
    out, ha, wa = layer(s, p)
    assert ha is None and wa is None and out.requires_grad
    out.backward(d_out.cuda())
    for k, v in layer.named_parameters():
        assert v.grad.shape == v.shape and v.grad.dtype == v.dtype
    return dict(out=out.detach().cpu(), d_src=s.grad.cpu(), d_pos=p.grad.cpu(), grads={k: v.grad.cpu() for k, v in layer.named_parameters()})


def case_option(name, request):
    """option train_valu for the case, back to 0 when the test ends"""
    from axial_vs_amd import _lib
    _lib.check(_lib.lib().axvs_set_option(b"train_valu", tc.CASES[name].valu), "axvs_set_option")
    request.addfinalizer(lambda: _lib.lib().axvs_set_option(b"train_valu", 0))


def kept_step(name):
    """the recompute = False step of the case, run once and shared by the tests below (the caller has set the case's option)"""
    if name not in _steps:
        _steps[name] = step(name, False)
    return _steps[name]


def differing(a, b):
    x, y = tc.tensors(a), tc.tensors(b)
    return [k for k in x if not torch.equal(x[k], y[k])]


@pytest.mark.parametrize("name", list(tc.CASES))
def test_training_at_the_tier_edges_vs_float64_oracle(name, request):
    case_option(name, request)
    c = tc.CASES[name]
    ref64, ref32 = tc.reference(name, torch.float64), tc.reference(name, torch.float32)
    got = kept_step(name)
    assert got["out"].shape == ref64["out"].shape and set(got["grads"]) == set(ref64["grads"])
    assert tc.all_finite(got), [k for k, v in tc.tensors(got).items() if not bool(torch.isfinite(v).all())]
    e = tc.errors(got, ref64)
    rs = tc.ratios(got, ref64, ref32)
    # the gradients that vanish in exact arithmetic: rounding noise on both sides, held to an absolute bound
    scale = tc.grad_scale(ref64)
    noise = {}
    for k in tc.vanishing(c):
        noise[k] = float(got["grads"][k].double().norm()) / scale
        LOG.append(f"{name} grad.{k} vanishes: device noise {noise[k]:.3e} of the largest gradient norm")
        del e["grad." + k], rs["grad." + k]
    for k, (r, dev, yard) in rs.items():
        LOG.append(f"{name} {k} r={r:.3g} device={dev:.3e} fp32_oracle={yard:.3e}")
    worst, rworst = max(e, key=e.get), max(rs, key=lambda k: rs[k][0])
    print(f"{name}: worst error {worst} {e[worst]:.2e}; worst ratio {rworst} r = {rs[rworst][0]:.3g} (device {rs[rworst][1]:.2e}, fp32 oracle "
          f"{rs[rworst][2]:.2e}); worst noise on a vanishing gradient {max(noise.values()):.2e}")
    assert e[worst] < TOL, {k: f"{v:.2e}" for k, v in e.items() if v >= TOL}
    assert max(noise.values()) <= tc.VANISH_NOISE * R_MARGIN, noise
    assert rs[rworst][0] <= R_MARGIN, {k: f"{v[0]:.3g}" for k, v in rs.items() if v[0] > R_MARGIN}


@pytest.mark.parametrize("name", list(tc.CASES))
def test_recompute_gives_the_bits_of_kept_activations(name, request):
    """recompute = True rebuilds the activations in the backward with the same kernels in the same order: out and every gradient
    carry the bits of the recompute = False step"""
    case_option(name, request)
    d = differing(kept_step(name), step(name, True))
    assert not d, d


@pytest.mark.parametrize("name", tc.TWICE)
def test_a_second_step_gives_the_same_bits(name, request):
    """fixed summation orders: two query chunks in the key-side backward, a second iteration of the VALU kernels' outer loops"""
    case_option(name, request)
    d = differing(kept_step(name), step(name, False))
    assert not d, d


def test_refusals_are_named():
    import axial_vs_amd as ax
    layer = ax.TemporalAxialTrajectoryAttentionLayer(64, 64, n_heads=8).cuda().train()
    src, pos = orc.synthetic_clip(1, 17, 64, 2, 2, 1)
    with pytest.raises(RuntimeError, match="T=17"):
        layer(src.cuda(), pos.cuda())
    # head_dim 64: 320 keys per frame ran above (full_d64_l320); 321 = 3 x 107 do not fit
    full = ax.TemporalTrajectoryAttentionLayer(128, 64, n_heads=2).cuda().train()
    src, pos = orc.synthetic_clip(1, 1, 128, 3, 107, 1)
    with pytest.raises(RuntimeError, match="head_dim=64"):
        full(src.cuda(), pos.cuda())
    axial = ax.TemporalAxialTrajectoryAttentionLayer(128, 64, n_heads=2).cuda().train()
    src, pos = orc.synthetic_clip(1, 1, 128, 1, 321, 1)
    with pytest.raises(RuntimeError, match="axis length too long"):
        axial(src.cuda(), pos.cuda())


def test_zz_report():
    """Last in the file: the measured ratios of this run, one line per case and tensor (written to $AXVS_TRAJ_TRAIN_PARITY_OUT when
    that is set)."""
    print("\n".join(LOG))
    path = os.environ.get("AXVS_TRAJ_TRAIN_PARITY_OUT")
    if path and LOG:          # (no case ran, as under -k: leave a file that is there alone)
        with open(path, "w") as f:
            f.write("\n".join(LOG) + "\n")
