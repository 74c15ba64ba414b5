"""GPU: the training tier of the full T*H*W layer (TemporalTrajectoryAttentionLayer, temporal_attn_type="trajectory",
WC/temporal_attention.py:103-155) -- forward + backward through the C-ABI against autograd on the float64 oracle, composed here
from orc.trajectory_attention and the hash dropout of include/axvs.h (sites 1, 2, 5, 6)."""
import pytest
import torch

import __graft_entry__ as ge
import axvs_oracle as orc
from golden_util import rel_err, rel_l2
from traj_train_cases import traj_layer_train_ref

pytestmark = pytest.mark.gpu

TOL = 1e-4


@pytest.fixture(scope="module", autouse=True)
def built():
    ge.build()
    assert torch.cuda.is_available()


def traj_shapes(C, F):
    return {k.replace("height_attn", "temporal_attn"): v for k, v in orc.axial_layer_param_shapes(C, F).items() if "width_attn" not in k}


def make_layer(C, F, w, p_dropout, p_attn_drop, seed, heads=8, **kw):
    import axial_vs_amd as ax
    layer = ax.TemporalTrajectoryAttentionLayer(C, F, dropout=p_dropout, attn_drop=p_attn_drop, n_heads=heads, **kw)
    layer.load_state_dict(w, strict=True)
    layer = layer.cuda().train()
    layer.dropout_seed = seed
    return layer


def run(layer, src, pos, d_out):
    s = src.float().cuda().requires_grad_(True)
    p = pos.float().cuda().requires_grad_(True)
    out, ha, wa = layer(s, p)
    assert ha is None and wa is None and out.requires_grad
    out.backward(d_out.float().cuda())
    return out.detach().cpu(), s.grad.cpu(), p.grad.cpu(), {k: v.grad.cpu() for k, v in layer.named_parameters()}


def grad_errors(grads, wd):
    scale = max(float(v.grad.norm()) for v in wd.values())
    return {k: float((grads[k].double() - wd[k].grad).norm() / max(float(wd[k].grad.norm()), 1e-3 * scale)) for k in wd}


# (B, T, C, H, W, F): head_dim 8 on the VALU kernels (63 keys); <= 128 keys (split kernel); 240 keys (LDS-resident MFMA);
# 600 and 575 keys (chunked-key kernels, not multiples of 16)
@pytest.mark.parametrize("recompute", [False, True])
@pytest.mark.parametrize("shape,p_drop,p_attn", [((2, 3, 64, 7, 9, 128), 0.1, 0.1), ((1, 2, 256, 8, 12, 512), 0.3, 0.0),
                                                 ((1, 4, 256, 12, 20, 1024), 0.0, 0.0), ((1, 2, 256, 24, 25, 512), 0.1, 0.3),
                                                 ((1, 3, 256, 25, 23, 256), 0.0, 0.1)])
def test_full_layer_training_vs_float64_oracle_autograd(shape, p_drop, p_attn, recompute):
    B, T, C, H, W, F = shape
    w = orc.random_weights(traj_shapes(C, F), 71)
    src, pos = orc.synthetic_clip(B, T, C, H, W, 71)
    d_out = torch.randn(B * T, H * W, C, generator=torch.Generator().manual_seed(72))
    seed = 31337
    wd = {k: v.double().requires_grad_(True) for k, v in w.items()}
    sd, pd = src.double().requires_grad_(True), pos.double().requires_grad_(True)
    ref = traj_layer_train_ref(sd, pd, wd, 8, p_drop, p_attn, seed)
    ref.backward(d_out.double())
    layer = make_layer(C, F, w, p_drop, p_attn, seed)
    layer.recompute = recompute
    out, d_src, d_pos, grads = run(layer, src, pos, d_out)
    e = dict(out=rel_err(out, ref.detach()), d_src=rel_err(d_src, sd.grad), d_pos=rel_err(d_pos, pd.grad),
             out_l2=rel_l2(out, ref.detach()), d_src_l2=rel_l2(d_src, sd.grad))
    pe = grad_errors(grads, wd)
    print(f"{shape} p=({p_drop},{p_attn}) recompute={recompute}: {e} worst parameter gradient {max(pe.values()):.2e}")
    assert max(e.values()) < TOL, e
    assert max(pe.values()) < TOL, pe
    for k, p in layer.named_parameters():
        assert p.grad.shape == p.shape and p.grad.dtype == p.dtype


def test_trajectory_encoder_trains():
    """TemporalEncoder("trajectory") -- the reference encoder's default type -- with two layers in train() mode."""
    import axial_vs_amd as ax
    B, T, C, H, W, F = 1, 2, 256, 20, 30, 512            # 600 keys per frame: the chunked kernels
    enc = ax.TemporalEncoder(C, F, dropout=0.1, attn_drop=0.1, n_heads=8, temporal_attn_type="trajectory", num_temporal_layer=2)
    ws = [orc.random_weights(traj_shapes(C, F), 90 + i) for i in range(2)]
    for i, layer in enumerate(enc.temporal_layers):
        layer.load_state_dict(ws[i], strict=True)
        layer.dropout_seed = 500 + i
    enc = enc.cuda().train()
    src, pos = orc.synthetic_clip(B, T, C, H, W, 91)
    s = src.cuda().requires_grad_(True)
    out = enc(s, pos.cuda())[0]
    out.square().sum().backward()
    wd = [{k: v.double().requires_grad_(True) for k, v in w.items()} for w in ws]
    sd = src.double().requires_grad_(True)
    y = sd
    for i in range(2):
        y = traj_layer_train_ref(y, pos.double(), wd[i], 8, 0.1, 0.1, 500 + i)
    y.square().sum().backward()
    assert rel_err(out.detach().cpu(), y.detach()) < TOL
    assert rel_err(s.grad.cpu(), sd.grad) < TOL
    for i in range(2):
        pe = grad_errors({k: v.grad.cpu() for k, v in enc.temporal_layers[i].named_parameters()}, wd[i])
        assert max(pe.values()) < TOL, (i, pe)


def test_long_frames_at_full_size_fit_in_memory():
    """[1,4,256,64,64] (4096 keys per frame): the reference's autograd holds > 17 GB for this layer; the tier a few hundred MB."""
    B, T, C, H, W, F = 1, 4, 256, 64, 64, 1024
    w = orc.random_weights(traj_shapes(C, F), 5)
    src, pos = orc.synthetic_clip(B, T, C, H, W, 5)
    layer = make_layer(C, F, w, 0.1, 0.1, 2024)
    s = src.cuda().requires_grad_(True)
    p = pos.cuda()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    out = layer(s, p)[0]
    out.square().mean().backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    print(f"[1,4,256,64,64] forward + backward: peak {peak / 2 ** 30:.2f} GiB")
    assert peak < 3 * 2 ** 30
    assert torch.isfinite(out).all() and torch.isfinite(s.grad).all()
    for k, v in layer.named_parameters():
        assert torch.isfinite(v.grad).all(), k
    assert float(s.grad.abs().max()) > 0


def test_train_mode_without_dropout_matches_eval_tier():
    """p = 0 at 64 x 48 = 3072 keys per frame: the fp32 training tier and the 16-bit inference tier compute the same function."""
    B, T, C, H, W, F = 1, 2, 256, 64, 48, 512
    w = orc.random_weights(traj_shapes(C, F), 81)
    src, pos = orc.synthetic_clip(B, T, C, H, W, 81)
    layer = make_layer(C, F, w, 0.0, 0.0, None)
    out_train = layer(src.cuda(), pos.cuda())[0].detach()
    with torch.no_grad():
        out_eval = layer.eval()(src.cuda(), pos.cuda())[0]
    assert not out_eval.requires_grad
    e = rel_err(out_eval.cpu(), out_train.cpu())
    print(f"train p=0 vs eval tier, 3072 keys per frame: {e:.2e}")
    assert e < 1e-3


def test_dropout_is_a_function_of_the_seed():
    B, T, C, H, W, F = 1, 2, 256, 24, 25, 256
    w = orc.random_weights(traj_shapes(C, F), 3)
    src, pos = orc.synthetic_clip(B, T, C, H, W, 3)
    d_out = torch.ones(B * T, H * W, C)
    a = run(make_layer(C, F, w, 0.3, 0.3, 7), src, pos, d_out)
    b = run(make_layer(C, F, w, 0.3, 0.3, 7), src, pos, d_out)
    c = run(make_layer(C, F, w, 0.3, 0.3, 8), src, pos, d_out)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert all(torch.equal(a[3][k], b[3][k]) for k in a[3])
    assert not torch.equal(a[0], c[0])
    layer = make_layer(C, F, w, 0.3, 0.3, None)
    torch.manual_seed(5)
    o1 = layer(src.cuda(), pos.cuda())[0]
    o2 = layer(src.cuda(), pos.cuda())[0]
    torch.manual_seed(5)
    o3 = layer(src.cuda(), pos.cuda())[0]
    assert not torch.equal(o1, o2) and torch.equal(o1, o3)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_amp_autocast_and_grad_scaling(dtype):
    """torch.autocast + a scaled loss: fp32 out, gradients in the inputs' dtypes, linear in the loss scale."""
    B, T, C, H, W, F = 1, 2, 256, 24, 25, 256
    w = orc.random_weights(traj_shapes(C, F), 13)
    src, pos = orc.synthetic_clip(B, T, C, H, W, 13)
    layer = make_layer(C, F, w, 0.1, 0.1, 99)
    res = {}
    for scale in (1.0, 256.0):
        layer.zero_grad()
        s = src.cuda().to(dtype).requires_grad_(True)
        with torch.autocast(device_type="cuda", dtype=dtype):
            out = layer(s, pos.cuda().to(dtype))[0]
            loss = out.float().square().sum() * scale       # (sum: gradients of O(1) -- normal numbers in fp16 at both scales)
        assert out.dtype == torch.float32
        loss.backward()
        assert s.grad.dtype == dtype
        res[scale] = (out.detach(), s.grad.float(), {k: v.grad.clone() for k, v in layer.named_parameters()})
        for v in layer.parameters():
            assert v.grad.dtype == torch.float32
    assert torch.equal(res[1.0][0], res[256.0][0])
    floor = 1e-3 * max(float(v.norm()) for v in res[1.0][2].values())     # (k.bias: its true gradient is 0, both sides hold rounding noise)
    for k in res[1.0][2]:
        if dtype == torch.bfloat16:      # a power-of-two loss scale scales every operation exactly: bit-exact multiples
            assert torch.equal(res[256.0][2][k] / 256.0, res[1.0][2][k]), k
        else:                            # fp16 pieces: the smallest products still meet fp16's subnormal range
            assert float((res[256.0][2][k] / 256.0 - res[1.0][2][k]).norm()) < 1e-3 * max(float(res[1.0][2][k].norm()), floor), k
    assert rel_l2(res[256.0][1].cpu() / 256.0, res[1.0][1].cpu()) < 1e-2


@pytest.mark.parametrize("C,heads,H,W,f32", [(256, 8, 24, 25, True), (256, 8, 8, 9, True), (256, 4, 12, 20, False), (256, 4, 6, 7, False)])
def test_eval_fp32_tier(C, heads, H, W, f32):
    """mfma_dtype='f32' (long and short frames) and head_dim 64 (256 / 4: the 16-bit kernels stop at 32) in eval mode: the training
    tier's forward with dropout off, within 1e-5 of the float64 oracle."""
    import axial_vs_amd as ax
    B, T, F = 1, 2, 256
    w = orc.random_weights(traj_shapes(C, F), 40 + H)
    src, pos = orc.synthetic_clip(B, T, C, H, W, 40 + H)
    layer = ax.TemporalTrajectoryAttentionLayer(C, F, dropout=0.1, attn_drop=0.1, n_heads=heads, mfma_dtype="f32" if f32 else None)
    layer.load_state_dict(w, strict=True)
    layer = layer.cuda().eval()
    assert layer._dtype() == "f32"
    with torch.no_grad():
        y = layer(src.cuda(), pos.cuda())[0].cpu()
    ref = orc.trajectory_layer(src.double(), pos.double(), {k: v.double() for k, v in w.items()}, heads)
    e = rel_err(y, ref)
    print(f"eval fp32 tier C={C} heads={heads} {H}x{W}: {e:.2e}")
    assert e < 1e-5


def test_head_dim_64_frame_bound_is_named():
    import axial_vs_amd as ax
    layer = ax.TemporalTrajectoryAttentionLayer(256, 256, n_heads=4).cuda().train()      # head_dim 64, 18 x 20 = 360 > 320 keys
    src, pos = orc.synthetic_clip(1, 2, 256, 18, 20, 1)
    with pytest.raises(RuntimeError, match="head_dim=64"):
        layer(src.cuda(), pos.cuda())
