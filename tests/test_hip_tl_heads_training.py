"""GPU: the training tier of the Tube-Link cross-clip head's prediction heads (axvs_tl_heads_train_*): post_norm, class pooling,
cls_embed, the mask MLP and the per-clip mask einsum of every layer in one library call behind TubeLinkCrossClipHead's train() mode.
Checked against autograd on the float64 oracle (orc.tl_cross_clip_head)."""
import pytest
import torch

import __graft_entry__ as ge
import axvs_oracle as orc
from golden_util import load, rel_err, rel_l2, weights

pytestmark = pytest.mark.gpu

TOL = 1e-4   # the bar of test_hip_cc_training.py: fp32 activations, split-bf16 GEMMs
FIXTURES = ["g6_tl_cc_head_Tc3_Q16_f2_L2", "g6_tl_cc_head_Tc2_Q20_f1_L1", "g6_tl_cc_head_Tc4_Q100_f2_L4"]
TORCH_OPS = ("aten::addmm", "aten::mm", "aten::bmm", "aten::linear", "aten::einsum", "aten::native_layer_norm", "aten::_softmax", "aten::relu",
             "aten::threshold_backward")


@pytest.fixture(scope="module", autouse=True)
def built():
    ge.build()
    assert torch.cuda.is_available()


def fixture_case(name):
    z, m = load(name)
    w = weights(z, m)
    g = torch.Generator().manual_seed(m["seed"] + 1)
    cq = torch.randn(m["B"], m["Tc"], m["Q"], 256, generator=g)
    mf = torch.nn.functional.normalize(torch.randn(m["B"], m["Tc"] * m["fpc"], m["Cm"], m["h"], m["w"], generator=g), dim=2)
    return dict(w=w, cq=cq, mf=mf, layers=m["layers"], K=m["num_classes"], Cm=m["Cm"], seed=m["seed"])


def seeded_case(B, Tc, Q, fpc, h, w, layers, K, Cm, seed):
    import axial_vs_amd as ax
    mod = ax.TubeLinkCrossClipHead(num_classes=K, out_channels=Cm, num_cc_layers=layers)
    wts = orc.random_weights({k: tuple(v.shape) for k, v in mod.state_dict().items()}, seed)
    g = torch.Generator().manual_seed(seed + 1)
    cq = torch.randn(B, Tc, Q, 256, generator=g)
    mf = torch.nn.functional.normalize(torch.randn(B, Tc * fpc, Cm, h, w, generator=g), dim=2)
    return dict(w=wts, cq=cq, mf=mf, layers=layers, K=K, Cm=Cm, seed=seed)


SEEDED = {
    "seeded_B2_Tc3_25x43": dict(B=2, Tc=3, Q=16, fpc=2, h=25, w=43, layers=2, K=12, Cm=256, seed=911),
    # Tc = 1: the class pooling's softmax over one clip, every ASPP tap on the row itself; Q = 4 the smallest; one pixel per frame
    "seeded_Tc1_Q4_1x1": dict(B=1, Tc=1, Q=4, fpc=1, h=1, w=1, layers=1, K=3, Cm=128, seed=912),
    # Tc = 16, the most the tier builds; three layers: with a mask-feature gradient tlt_sum_layers_kernel adds their shares; 15 pixels
    "seeded_Tc16_Q4_3x5_L3": dict(B=1, Tc=16, Q=4, fpc=1, h=3, w=5, layers=3, K=7, Cm=256, seed=913),
    # B = 3; Q = 132 = a whole 128-row tile plus 4 rows; 133 pixels per frame (odd, one tile plus 5); two frames per clip
    "seeded_B3_Q132_7x19_f2": dict(B=3, Tc=2, Q=132, fpc=2, h=7, w=19, layers=2, K=12, Cm=256, seed=914),
}


def make_head(k, p_drop=0.0, seed=None):
    import axial_vs_amd as ax
    mod = ax.TubeLinkCrossClipHead(num_classes=k["K"], out_channels=k["Cm"], num_cc_layers=k["layers"], trajectory_drop_out=p_drop,
                                   drop_path_prob=p_drop)
    mod.load_state_dict(k["w"], strict=True)
    mod = mod.cuda().train()
    if seed is not None:
        mod.dropout_seed = seed
    return mod


def cotangents(cls, masks, seed):
    g = torch.Generator().manual_seed(seed + 2)
    return [torch.randn(c.shape, generator=g) for c in cls], [torch.randn(x.shape, generator=g) * 0.05 for x in masks]


def compare(k, mf_grad=False):
    """One training step of the head against float64 autograd: outputs of every layer, d_clip_query, every parameter gradient and
    (mf_grad) d_mask_features -> dict of errors."""
    mod = make_head(k)
    q = k["cq"].cuda().requires_grad_(True)
    mf = k["mf"].cuda().requires_grad_(mf_grad)
    cls, masks = mod(q, mf)
    assert isinstance(cls, tuple) and isinstance(masks, tuple) and len(cls) == len(masks) == k["layers"]
    d_cls, d_masks = cotangents(cls, masks, k["seed"])
    (sum((a * b.cuda()).sum() for a, b in zip(cls, d_cls)) + sum((a * b.cuda()).sum() for a, b in zip(masks, d_masks))).backward()
    wd = {n: v.double().requires_grad_(True) for n, v in k["w"].items()}
    qd = k["cq"].double().requires_grad_(True)
    mfd = k["mf"].double().requires_grad_(mf_grad)
    rc, rm = orc.tl_cross_clip_head(qd, mfd, wd, k["layers"])
    (sum((a * b.double()).sum() for a, b in zip(rc, d_cls)) + sum((a * b.double()).sum() for a, b in zip(rm, d_masks))).backward()
    e = {}
    for i in range(k["layers"]):
        e[f"cls{i}"] = rel_err(cls[i].detach().cpu(), rc[i].detach())
        e[f"masks{i}"] = rel_err(masks[i].detach().cpu(), rm[i].detach())
    e["d_clip_query"] = rel_err(q.grad.cpu(), qd.grad)
    if mf_grad:
        e["d_mask_features"] = rel_err(mf.grad.cpu(), mfd.grad)
    scale = max(float(v.grad.norm()) for v in wd.values() if v.grad is not None)
    for n, p in mod.named_parameters():
        assert p.grad is not None, n
        e[n] = float((p.grad.cpu().double() - wd[n].grad).norm() / max(float(wd[n].grad.norm()), 1e-3 * scale))
    return e


@pytest.mark.parametrize("name", FIXTURES + list(SEEDED))
def test_heads_tier_matches_float64_autograd(name):
    k = fixture_case(name) if name in FIXTURES else seeded_case(**SEEDED[name])
    e = compare(k)
    worst = max(e, key=e.get)
    print(f"{name}: worst {worst} {e[worst]:.2e}; d_clip_query {e['d_clip_query']:.2e}")
    assert max(e.values()) < TOL, {n: f"{v:.2e}" for n, v in e.items() if v >= TOL}


@pytest.mark.parametrize("name", ["g6_tl_cc_head_Tc2_Q20_f1_L1", "seeded_B2_Tc3_25x43", "seeded_Tc16_Q4_3x5_L3", "seeded_B3_Q132_7x19_f2"])
def test_mask_feature_gradient(name):
    """d_mask_features when the pixel features want a gradient: one layer (written directly), two and three layers (shares added in
    order)."""
    k = fixture_case(name) if name in FIXTURES else seeded_case(**SEEDED[name])
    e = compare(k, mf_grad=True)
    print(f"{name}: d_mask_features {e['d_mask_features']:.2e}")
    assert max(e.values()) < TOL, {n: f"{v:.2e}" for n, v in e.items() if v >= TOL}


def recorded_ops(step):
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU]) as prof:
        step()
    torch.cuda.synchronize()
    return {e.key for e in prof.key_averages()}


def test_head_step_runs_no_torch_linear_layernorm_softmax_relu_or_einsum():
    k = fixture_case("g6_tl_cc_head_Tc3_Q16_f2_L2")
    mod = make_head(k)
    q = k["cq"].cuda().requires_grad_(True)
    mf = k["mf"].cuda()

    def step():
        cls, masks = mod(q, mf)
        (sum(c.square().sum() for c in cls) + sum(x.square().sum() for x in masks)).backward()
    names = recorded_ops(step)
    assert not any(n in names for n in TORCH_OPS), sorted(n for n in names if n in TORCH_OPS)
    assert all(p.grad is not None for p in mod.parameters())


def test_dropout_steps_are_bit_reproducible():
    k = fixture_case("g6_tl_cc_head_Tc4_Q100_f2_L4")
    runs = []
    for _ in range(2):
        mod = make_head(k, 0.1, 1234)
        q = k["cq"].cuda().requires_grad_(True)
        cls, masks = mod(q, k["mf"].cuda())
        d_cls, d_masks = cotangents(cls, masks, 5)
        (sum((a * b.cuda()).sum() for a, b in zip(cls, d_cls)) + sum((a * b.cuda()).sum() for a, b in zip(masks, d_masks))).backward()
        runs.append(([c.detach() for c in cls], [x.detach() for x in masks], q.grad, {n: p.grad for n, p in mod.named_parameters()}))
    (c1, m1, q1, g1), (c2, m2, q2, g2) = runs
    assert all(torch.equal(a, b) for a, b in zip(c1, c2)) and all(torch.equal(a, b) for a, b in zip(m1, m2))
    assert torch.equal(q1, q2) and all(torch.equal(g1[n], g2[n]) for n in g1)
    ref = make_head(k, 0.0)
    cls0, _ = ref(k["cq"].cuda(), k["mf"].cuda())
    assert not torch.equal(cls0[-1].detach(), c1[-1])          # the dropout does act


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_amp_autocast_and_grad_scaling(dtype):
    """torch.autocast + a scaled loss: fp32 outputs, gradients in the inputs' dtypes and linear in the loss scale, within 5e-2
    (relative L2) of the fp32 tier."""
    k = fixture_case("g6_tl_cc_head_Tc3_Q16_f2_L2")
    cq16, mf16 = k["cq"].cuda().to(dtype), k["mf"].cuda().to(dtype)

    def step(amp, scale):
        mod = make_head(k)
        q = (cq16 if amp else cq16.float()).clone().requires_grad_(True)
        mf = (mf16 if amp else mf16.float()).clone().requires_grad_(True)
        with torch.autocast(device_type="cuda", dtype=dtype, enabled=amp):
            cls, masks = mod(q, mf)
            loss = (sum(c.float().square().sum() for c in cls) + sum(x.float().square().sum() for x in masks)) * scale
        assert all(c.dtype == torch.float32 for c in cls) and all(x.dtype == torch.float32 for x in masks)
        loss.backward()
        assert q.grad.dtype == q.dtype and mf.grad.dtype == mf.dtype
        assert all(p.grad.dtype == torch.float32 for p in mod.parameters())
        return (torch.stack([x.detach() for x in masks]).cpu(), q.grad.float().cpu() / scale, mf.grad.float().cpu() / scale,
                {n: p.grad.cpu() / scale for n, p in mod.named_parameters()})

    m1, q1, f1, g1 = step(True, 1.0)
    m256, q256, f256, g256 = step(True, 256.0)
    m32, q32, f32, g32 = step(False, 1.0)
    assert torch.equal(m1, m256)
    floor = 1e-3 * max(float(v.norm()) for v in g1.values())
    for n in g1:
        assert float((g256[n] - g1[n]).norm()) < 1e-3 * max(float(g1[n].norm()), floor), n
    assert rel_l2(q256, q1) < 1e-2 and rel_l2(f256, f1) < 1e-2
    scale = max(float(v.norm()) for v in g32.values())
    e_w = max(float((g1[n] - g32[n]).norm()) / max(float(g32[n].norm()), 1e-2 * scale) for n in g32)
    e = dict(masks=rel_l2(m1, m32), d_clip_query=rel_l2(q1, q32), d_mask_features=rel_l2(f1, f32), worst_param_grad=e_w)
    print(f"Tube-Link head under {dtype} autocast vs the fp32 tier (relative L2):", {n: f"{v:.2e}" for n, v in e.items()})
    assert max(e.values()) < 5e-2, e


def test_refused_configuration_keeps_the_torch_heads():
    """Q = 10 is outside the heads' bounds (Q a multiple of 4): the chain still runs on the tier, the heads as torch modules."""
    from axial_vs_amd import _lib
    from axial_vs_amd.cc_training import tl_heads_cfg, tl_heads_supported
    assert not tl_heads_supported(tl_heads_cfg(2, 1, 10, 3, 2, 9, 11, 8, 128))
    assert "Q=10" in _lib.lib().axvs_last_error().decode()
    k = seeded_case(B=1, Tc=3, Q=10, fpc=2, h=9, w=11, layers=2, K=7, Cm=128, seed=77)
    e = compare(k, mf_grad=True)
    worst = max(e, key=e.get)
    print(f"Q=10 through the torch heads: worst {worst} {e[worst]:.2e}")
    assert max(e.values()) < TOL, {n: f"{v:.2e}" for n, v in e.items() if v >= TOL}
