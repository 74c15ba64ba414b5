"""GPU: the training tier of MSDeformAttnTransformerEncoderLayer (WC/msdeformattn.py:177-216; axvs_msda_layer_train_fwd / _bwd) --
forward + backward against float64 autograd on a restatement built from the oracle's deformable attention and the hash dropout of
include/axvs.h (sites 7, 8, 9), recompute, AMP, the profiler (no torch Linear / LayerNorm / softmax / dropout kernels in the layer or
the within-clip module's train step) and the fallback to the torch composition."""
import pytest
import torch

import __graft_entry__ as ge
import axvs_oracle as orc
from golden_util import rel_err, rel_l2

pytestmark = pytest.mark.gpu

TOL = 1e-4
TORCH_OPS = ("aten::addmm", "aten::mm", "aten::linear", "aten::native_layer_norm", "aten::_softmax", "aten::native_dropout")


@pytest.fixture(scope="module", autouse=True)
def built():
    ge.build()
    assert torch.cuda.is_available()


def layer_weights(C, F, M, L, P, seed):
    shapes = {"self_attn.sampling_offsets.weight": (M * L * P * 2, C), "self_attn.sampling_offsets.bias": (M * L * P * 2,),
              "self_attn.attention_weights.weight": (M * L * P, C), "self_attn.attention_weights.bias": (M * L * P,),
              "self_attn.value_proj.weight": (C, C), "self_attn.value_proj.bias": (C,), "self_attn.output_proj.weight": (C, C),
              "self_attn.output_proj.bias": (C,), "norm1.weight": (C,), "norm1.bias": (C,), "linear1.weight": (F, C), "linear1.bias": (F,),
              "linear2.weight": (C, F), "linear2.bias": (C,), "norm2.weight": (C,), "norm2.bias": (C,)}
    w = orc.random_weights(shapes, seed)
    w["self_attn.sampling_offsets.bias"] = w["self_attn.sampling_offsets.bias"] * 20.0      # offsets of a few pixels
    return w


def msda_layer_train_ref(src, pos, ref_pts, shapes, w, M, L, P, pad, p, seed):
    """The layer's forward in train() mode with the tier's dropout factors: differentiable torch code."""
    N, S, C = src.shape
    F = w["linear1.weight"].shape[0]
    dt = src.dtype
    a = orc.msda_module(src + pos, ref_pts, src, shapes, orc._sub(w, "self_attn"), M, L, P, pad)
    x = orc._layer_norm(src + a * orc.dropout_keep(seed, 7, N * S * C, p, dt).reshape(N, S, C), w, "norm1")
    r = torch.relu(orc._linear(x, w, "linear1")) * orc.dropout_keep(seed, 8, N * S * F, p, dt).reshape(N, S, F)
    ff = orc._linear(r, w, "linear2") * orc.dropout_keep(seed, 9, N * S * C, p, dt).reshape(N, S, C)
    return orc._layer_norm(x + ff, w, "norm2")


def case(N, C, shapes, mask, ref_dim, seed=71):
    M, P, F = 8, 4, 2 * C
    L, S = len(shapes), sum(h * w for h, w in shapes)
    w = layer_weights(C, F, M, L, P, seed)
    g = torch.Generator().manual_seed(seed + 1)
    src, pos = torch.randn(N, S, C, generator=g), torch.randn(N, S, C, generator=g) * 0.5
    if ref_dim == 2:
        ref_pts = torch.rand(N, S, L, 2, generator=g)
    else:
        ref_pts = torch.cat([torch.rand(N, S, L, 2, generator=g), 0.1 + 0.3 * torch.rand(N, S, L, 2, generator=g)], -1)
    pad = (torch.rand(N, S, generator=g) < 0.1) if mask else None
    d_out = torch.randn(N, S, C, generator=g)
    return dict(C=C, F=F, M=M, L=L, P=P, shapes=shapes, w=w, src=src, pos=pos, ref=ref_pts, pad=pad, d_out=d_out)


def make_layer(k, p, seed, train=True):
    import axial_vs_amd as ax
    layer = ax.MSDeformAttnTransformerEncoderLayer(k["C"], k["F"], dropout=p, n_levels=k["L"], n_heads=k["M"], n_points=k["P"])
    layer.load_state_dict(k["w"], strict=True)
    layer = layer.cuda().train(train)
    layer.dropout_seed = seed
    return layer


def run(layer, k, dtype=torch.float32):
    s = k["src"].cuda().to(dtype).requires_grad_(True)
    p = k["pos"].cuda().to(dtype).requires_grad_(True)
    out = layer(s, p, k["ref"].cuda(), torch.as_tensor(k["shapes"]).cuda(), None, k["pad"].cuda() if k["pad"] is not None else None)
    out.backward(k["d_out"].cuda())
    return out.detach().cpu(), s.grad.cpu(), p.grad.cpu(), {n: v.grad.detach().cpu().clone() for n, v in layer.named_parameters()}


def reference(k, p, seed):
    wd = {n: v.double().requires_grad_(True) for n, v in k["w"].items()}
    sd, pd = k["src"].double().requires_grad_(True), k["pos"].double().requires_grad_(True)
    ref = msda_layer_train_ref(sd, pd, k["ref"].double(), k["shapes"], wd, k["M"], k["L"], k["P"], k["pad"], p, seed)
    ref.backward(k["d_out"].double())
    return ref.detach(), sd.grad, pd.grad, wd


def grad_errors(grads, wd):
    scale = max(float(v.grad.norm()) for v in wd.values())
    return {n: float((grads[n].double() - wd[n].grad).norm() / max(float(wd[n].grad.norm()), 1e-3 * scale)) for n in wd}


SHAPES = [(2, 256, [(16, 12), (8, 6), (4, 3)]), (1, 64, [(6, 5), (3, 3)])]     # those of test_msda_encoder_layer_trains


@pytest.mark.parametrize("ref_dim", [2, 4])
@pytest.mark.parametrize("mask", [True, False])
@pytest.mark.parametrize("N,C,shapes", SHAPES)
def test_dropout_training_vs_float64_oracle_autograd(N, C, shapes, mask, ref_dim):
    """dropout 0.1 with a fixed dropout_seed in train() mode: output, d_src, d_pos and all 16 parameter gradients against float64 autograd
    on the restatement with orc.dropout_keep masks at sites 7, 8, 9."""
    k = case(N, C, shapes, mask, ref_dim)
    seed = 4242
    ref, d_src_ref, d_pos_ref, wd = reference(k, 0.1, seed)
    layer = make_layer(k, 0.1, seed)
    out, d_src, d_pos, grads = run(layer, k)
    e = dict(out=rel_err(out, ref), d_src=rel_err(d_src, d_src_ref), d_pos=rel_err(d_pos, d_pos_ref))
    pe = grad_errors(grads, wd)
    assert len(pe) == 16
    print(f"N={N} C={C} mask={mask} ref_dim={ref_dim}: {e} worst parameter gradient {max(pe, key=pe.get)} {max(pe.values()):.2e}")
    assert max(e.values()) < TOL and max(pe.values()) < TOL, (e, pe)
    for n, v in layer.named_parameters():
        assert v.grad.shape == v.shape and v.grad.dtype == v.dtype


def test_eval_mode_gradients_run_the_tier_without_dropout():
    k = case(2, 256, SHAPES[0][2], True, 2, seed=9)
    ref, d_src_ref, d_pos_ref, wd = reference(k, 0.0, 0)
    layer = make_layer(k, 0.1, None, train=False)
    out, d_src, d_pos, grads = run(layer, k)
    assert rel_err(out, ref) < TOL and rel_err(d_src, d_src_ref) < TOL and rel_err(d_pos, d_pos_ref) < TOL
    assert max(grad_errors(grads, wd).values()) < TOL


def test_recompute_matches_kept_activations():
    """recompute=True rebuilds the activations in the backward: the same bits as keeping them -- except where the core op's value
    gradient enters (value_proj's gradients and d_src): it accumulates by atomic adds in no fixed order, so those agree to rounding."""
    k = case(2, 256, SHAPES[0][2], True, 2)
    layer = make_layer(k, 0.1, 77)
    a = run(layer, k)
    layer.zero_grad()
    layer.recompute = True
    b = run(layer, k)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
    assert rel_err(b[1], a[1]) < 1e-5
    for n in a[3]:
        if n.startswith("self_attn.value_proj"):
            assert rel_err(b[3][n], a[3][n]) < 1e-5, n
        else:
            assert torch.equal(a[3][n], b[3][n]), n


def test_dropout_is_a_function_of_the_seed():
    k = case(1, 64, SHAPES[1][2], False, 2)
    o1 = run(make_layer(k, 0.3, 7), k)[0]
    o2 = run(make_layer(k, 0.3, 7), k)[0]
    o3 = run(make_layer(k, 0.3, 8), k)[0]
    assert torch.equal(o1, o2) and not torch.equal(o1, o3)


def recorded_ops(step):
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU]) as prof:
        step()
    torch.cuda.synchronize()
    return {e.key for e in prof.key_averages()}


def test_layer_step_runs_no_torch_linear_layernorm_softmax_or_dropout():
    k = case(2, 256, SHAPES[0][2], True, 2)
    layer = make_layer(k, 0.1, 5)
    names = recorded_ops(lambda: run(layer, k))
    assert not any(n in names for n in TORCH_OPS), sorted(n for n in names if n in TORCH_OPS)


def test_within_clip_module_train_step_runs_no_torch_linear_layernorm_softmax_or_dropout():
    from test_cabi_cpu import _decoder_from_meta
    from golden_util import load, weights
    z, m = load("g8_pixel_decoder_T2_S2")
    mod = _decoder_from_meta(dict(m))
    mod.within_clip_tracking_module.load_state_dict(weights(z, m), strict=True)
    mod = mod.cuda().train()
    g = torch.Generator().manual_seed(m["seed"] + 1)
    feats = {k: torch.randn(m["B"] * m["T"], m["chans"][k], *m["sizes"][k], generator=g).cuda().requires_grad_(True) for k in m["chans"]}

    def step():
        out, _, _ = mod.forward_features(dict(feats))
        sum(o.float().sum() for o in out.values()).backward()
    names = recorded_ops(step)
    assert not any(n in names for n in TORCH_OPS), sorted(n for n in names if n in TORCH_OPS)
    assert all(p.grad is not None for p in mod.parameters())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_amp_autocast_and_grad_scaling(dtype):
    """torch.autocast + a scaled loss: fp32 out, gradients in the inputs' dtypes, linear in the loss scale; with amp_compute = False
    the step equals the fp32 step on the same 16-bit-representable inputs."""
    k = case(2, 256, SHAPES[0][2], True, 2)
    layer = make_layer(k, 0.1, 99)
    ref_pts, ss, pad = k["ref"].cuda(), torch.as_tensor(k["shapes"]).cuda(), k["pad"].cuda()
    res = {}
    for scale in (1.0, 256.0):
        layer.zero_grad()
        s = k["src"].cuda().to(dtype).requires_grad_(True)
        p = k["pos"].cuda().to(dtype).requires_grad_(True)
        with torch.autocast(device_type="cuda", dtype=dtype):
            out = layer(s, p, ref_pts, ss, None, pad)
            loss = out.float().square().sum() * scale
        assert out.dtype == torch.float32
        loss.backward()
        assert s.grad.dtype == dtype and p.grad.dtype == dtype
        for v in layer.parameters():
            assert v.grad.dtype == torch.float32
        res[scale] = (out.detach(), s.grad.float(), {n: v.grad.clone() for n, v in layer.named_parameters()})
    assert torch.equal(res[1.0][0], res[256.0][0])
    floor = 1e-3 * max(float(v.norm()) for v in res[1.0][2].values())
    for n in res[1.0][2]:
        a, b = res[256.0][2][n] / 256.0, res[1.0][2][n]
        if dtype == torch.bfloat16 and not n.startswith("self_attn.value_proj"):   # (value_proj: atomic adds in the core op)
            assert torch.equal(a, b), n
        else:
            assert float((a - b).norm()) < 1e-3 * max(float(b.norm()), floor), n
    assert rel_l2(res[256.0][1].cpu() / 256.0, res[1.0][1].cpu()) < 1e-2
    # amp_compute = False: split-precision products under autocast -- the boundary alone is under test
    layer.amp_compute = False
    layer.zero_grad()
    s32 = k["src"].cuda().to(dtype).float().requires_grad_(True)
    p32 = k["pos"].cuda().to(dtype).float()
    out32 = layer(s32, p32, ref_pts, ss, None, pad)
    out32.sum().backward()
    g32 = {n: v.grad.clone() for n, v in layer.named_parameters()}
    layer.zero_grad()
    s16 = k["src"].cuda().to(dtype).requires_grad_(True)
    with torch.autocast(device_type="cuda", dtype=dtype):
        out = layer(s16, k["pos"].cuda().to(dtype), ref_pts, ss, None, pad)
        loss = out.sum() * 1024.0
    assert out.dtype == torch.float32
    assert torch.equal(out.detach(), out32.detach())
    loss.backward()
    for n, v in layer.named_parameters():
        assert rel_l2(v.grad.cpu() / 1024.0, g32[n].cpu()) < 1e-5 or float(g32[n].norm()) < 1e-4, n
    assert rel_l2(s16.grad.float().cpu() / 1024.0, s32.grad.cpu()) < 1e-2


def test_what_the_tier_does_not_cover_still_trains():
    """head_dim 12 (not built) and reference points that want a gradient run the torch composition, as before."""
    import axial_vs_amd as ax
    layer = ax.MSDeformAttnTransformerEncoderLayer(96, 192, dropout=0.0, n_levels=2, n_heads=8, n_points=4).cuda().train()
    s = torch.randn(1, 39, 96, device="cuda", requires_grad=True)
    ref_pts = torch.rand(1, 39, 2, 2, device="cuda")
    layer(s, torch.zeros_like(s), ref_pts, [(6, 5), (3, 3)]).sum().backward()
    assert torch.isfinite(s.grad).all() and all(v.grad is not None for v in layer.parameters())
    k = case(1, 64, SHAPES[1][2], False, 2)
    layer = make_layer(k, 0.0, 1)
    r = k["ref"].cuda().requires_grad_(True)
    out = layer(k["src"].cuda(), k["pos"].cuda(), r, k["shapes"])
    out.sum().backward()
    assert r.grad is not None and torch.isfinite(r.grad).all()
