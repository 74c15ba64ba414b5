"""GPU: the within-clip training tier's attention kernels at large and at almost one-hot softmax logits (tests/traj_train_regime_cases.py:
the regimes shift, sharp_s and sharp_t on cases of traj_train_cases.py, screened on the CPU) -- one training step of
TemporalAxialTrajectoryAttentionLayer / TemporalTrajectoryAttentionLayer per (case, regime), forward + backward through the C-ABI,
against autograd on the float64 oracle.

Per pair: everything finite; the ratio r of traj_train_cases (the device's distance from float64 in units of the fp32 oracle's) at
most R_MARGIN = 128, the bound of test_hip_traj_train_cases.py; every measure of traj_train_cases.errors at most max(TOL, 8 x the fp32
oracle's same measure); the gradients that vanish in exact arithmetic under max(VANISH_NOISE, the fp32 oracle's noise) * R_MARGIN
(traj_train_regime_cases.missed).  shift: out, d_src and d_pos also agree with the device's own step on the unshifted weights, within
8 x what the fp32 oracle's two steps differ by.  recompute = True and a second step give the same bits on the two sharp_s cases with
two query chunks / three key chunks.  The eval forward of mfma_dtype="f32" runs the same forward kernels and is held to R_MARGIN on
out.  test_zz_report lists r per pair and tensor (profiles/traj_train_regimes_parity.txt is that list from an MI355X)."""
import os

import pytest
import torch

import __graft_entry__ as ge
import axvs_oracle as orc
import traj_train_regime_cases as rc

pytestmark = pytest.mark.gpu

R_MARGIN = 128.0
assert rc.R_MARGIN == R_MARGIN and rc.TOL == 1e-4
# Measured on an MI355X over the 27 pairs, every line in profiles/traj_train_regimes_parity.txt: the largest r is 24.4 in shift
# (full_chunk769, linear1.bias), 20.7 in sharp_s (axial_t1, width_attn.v.bias), 28.3 in sharp_t (full_chunk769, norm1.weight), a bias or
# norm gradient (a column sum) as at ordinary inputs; no tensor needs a bound of its own.
R_MEASURED = dict(shift=24.4, sharp_s=20.7, sharp_t=28.3)
BITS = (("axial_t16_kv_two_chunks", "sharp_s"), ("full_chunk561", "sharp_s"))
EVAL_F32 = [(n, r) for n in ("axial_t8", "axial_d64_t7") for r in rc.REGIMES]
LOG = []
_steps = {}


@pytest.fixture(scope="module", autouse=True)
def built():
    ge.build()
    assert torch.cuda.is_available()


def step(name, regime, recompute=False, shifted=True):
    """one training step of the pair on the device (shifted = False: the pair's seed with the weights as drawn) -> result dict in the
    form of traj_train_cases.reference"""
    import axial_vs_amd as ax
    c, w = rc.pair_case(name, regime)
    if not shifted:
        w = rc.regime_weights(c, None, None)
    src, pos, d_out = rc.make_inputs(c)
    cls = ax.TemporalAxialTrajectoryAttentionLayer if c.kind == "axial" else ax.TemporalTrajectoryAttentionLayer
    layer = cls(c.C, c.F, dropout=c.p_dropout, attn_drop=c.p_attn_drop, n_heads=c.heads)
    layer.load_state_dict(w, strict=True)
    layer = layer.cuda().train()
    layer.dropout_seed = rc.dropout_seed(c)
    layer.recompute = recompute
    s, p = src.cuda().requires_grad_(True), pos.cuda().requires_grad_(True)
    out, ha, wa = layer(s, p)
    assert ha is None and wa is None and out.requires_grad
    out.backward(d_out.cuda())
    return dict(out=out.detach().cpu(), d_src=s.grad.cpu(), d_pos=p.grad.cpu(), grads={k: v.grad.cpu() for k, v in layer.named_parameters()})


def kept_step(name, regime):
    """the recompute = False step of the pair, run once and shared by the tests below"""
    if (name, regime) not in _steps:
        _steps[name, regime] = step(name, regime)
    return _steps[name, regime]


def differing(a, b):
    x, y = rc.tensors(a), rc.tensors(b)
    return [k for k in x if not torch.equal(x[k], y[k])]


@pytest.mark.parametrize("name,regime", rc.pair_ids())
def test_training_step_vs_float64_oracle(name, regime):
    c, _ = rc.pair_case(name, regime)
    ref64, ref32 = rc.reference(name, regime, torch.float64), rc.reference(name, regime, torch.float32)
    got = kept_step(name, regime)
    assert got["out"].shape == ref64["out"].shape and set(got["grads"]) == set(ref64["grads"])
    lines = []
    misses = rc.missed(c, got, ref64, ref32, lines, f"{name} {regime}")
    LOG.extend(lines)
    print("\n".join(lines))
    assert not misses, misses


@pytest.mark.parametrize("name", list(rc.FAMILY))
def test_shift_leaves_the_device_step_unchanged(name):
    """a constant on all logits of a softmax: the device's out, d_src and d_pos are those of its own step on the unshifted weights,
    within 8 x what the fp32 oracle's two steps differ by (max-norm, per tensor)"""
    got, base = kept_step(name, "shift"), step(name, "shift", shifted=False)
    o1, o0 = rc.reference(name, "shift", torch.float32), rc.plain(name, "shift", torch.float32)
    bad = {}
    for k in ("out", "d_src", "d_pos"):
        d, yard = float((got[k].double() - base[k].double()).abs().max()), float((o1[k].double() - o0[k].double()).abs().max())
        LOG.append(f"{name} shift {k} device shifted - unshifted {d:.3e} fp32_oracle {yard:.3e}")
        print(LOG[-1])
        if not d <= rc.ORACLE_FACTOR * yard:
            bad[k] = (d, yard)
    assert not bad, bad


@pytest.mark.parametrize("name,regime", BITS)
def test_recompute_and_a_second_step_give_the_same_bits(name, regime):
    kept = kept_step(name, regime)
    d = differing(kept, step(name, regime, recompute=True))
    assert not d, d
    d = differing(kept, step(name, regime))
    assert not d, d


@pytest.mark.parametrize("name,regime", EVAL_F32)
def test_f32_eval_forward_vs_float64_oracle(name, regime):
    """mfma_dtype="f32" in eval mode: the training tier's forward kernels without dropout, against orc.axial_layer in float64 with the
    same function in float32 as the yardstick"""
    import axial_vs_amd as ax
    c, w = rc.pair_case(name, regime)
    src, pos, _ = rc.make_inputs(c)
    ref64 = orc.axial_layer(src.double(), pos.double(), {k: v.double() for k, v in w.items()}, c.heads, want_attn=False)[0]
    ref32 = orc.axial_layer(src, pos, w, c.heads, want_attn=False)[0]
    layer = ax.TemporalAxialTrajectoryAttentionLayer(c.C, c.F, dropout=c.p_dropout, attn_drop=c.p_attn_drop, n_heads=c.heads, mfma_dtype="f32").eval()
    layer.load_state_dict(w, strict=True)
    with torch.no_grad():
        out = layer.cuda()(src.cuda(), pos.cuda())[0].cpu()
    assert bool(torch.isfinite(out).all())
    yard = max(float((ref32.double() - ref64).abs().max()), rc.tc.FLOOR * float(ref64.abs().max()))
    dev = float((out.double() - ref64).abs().max())
    LOG.append(f"{name} {regime} eval_f32 out r={dev / yard:.3g} device={dev:.3e} fp32_oracle={yard:.3e}")
    print(LOG[-1])
    assert dev / yard <= R_MARGIN


def test_zz_report():
    """Last in the file: the measured ratios of this run, one line per case, regime and tensor (written to
    $AXVS_TRAJ_TRAIN_REGIMES_OUT when that is set)."""
    print("\n".join(LOG))
    path = os.environ.get("AXVS_TRAJ_TRAIN_REGIMES_OUT")
    if path and LOG:          # (no case ran, as under -k: leave a file that is there alone)
        with open(path, "w") as f:
            f.write("\n".join(LOG) + "\n")
