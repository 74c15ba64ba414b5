"""Training step (forward + backward) of the full T*H*W layer (TemporalTrajectoryAttentionLayer) through the training tier at
[1,4,256,32,32] and [1,4,256,64,64]: ms per step and peak memory; --torch: the same step as torch fp32 autograd on the oracle's code
at [1,4,256,32,32] (the reference's own memory profile: T*HW x HW logits per frame)."""
import os, sys, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "oracle"))
import axvs_oracle as orc
import axial_vs_amd as ax

n = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 10
C, F, pd = 256, 1024, 0.1
shapes = {k.replace("height_attn", "temporal_attn"): v for k, v in orc.axial_layer_param_shapes(C, F).items() if "width_attn" not in k}


def timed(step):
    for _ in range(2):
        step()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    for _ in range(n):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3, torch.cuda.max_memory_allocated() / 2 ** 30


for H, W in ((32, 32), (64, 64)):
    for recompute in (False, True):
        layer = ax.TemporalTrajectoryAttentionLayer(C, F, dropout=pd, attn_drop=pd, n_heads=8)
        layer.load_state_dict(orc.random_weights(shapes, 1), strict=True)
        layer = layer.cuda().train()
        layer.recompute = recompute
        src, pos = orc.synthetic_clip(1, 4, C, H, W, 1)
        s, p = src.cuda().requires_grad_(True), pos.cuda()
        g = torch.randn_like(s)

        def step():
            layer(s, p)[0].backward(g)
        ms, gib = timed(step)
        print(f"[1,4,256,{H},{W}] recompute={recompute}: fwd+bwd {ms:.2f} ms/step, peak {gib:.2f} GiB", flush=True)
        del layer, s, p, g
        torch.cuda.empty_cache()

if "--torch" in sys.argv:
    H = W = 32
    w = {k: v.cuda().requires_grad_(True) for k, v in orc.random_weights(shapes, 1).items()}
    src, pos = orc.synthetic_clip(1, 4, C, H, W, 1)
    s, p = src.cuda().requires_grad_(True), pos.cuda()
    g = torch.randn_like(s)
    drop = torch.nn.Dropout(pd)

    def tstep():      # the reference's forward with torch's own dropout: attention map, attention output, FFN
        x = s.reshape(1, -1, C)
        kq = x + p.reshape(1, -1, C)
        keep = drop(torch.ones(1, 8, 4 * H * W, 4, H * W, device="cuda"))
        y, _ = orc.trajectory_attention(kq, kq, x, orc._sub(w, "temporal_attn"), 4, 8, want_attn=False, attn_keep=keep)
        z = orc._layer_norm((x + drop(y)).reshape(s.shape), w, "norm1")
        ff = drop(orc._linear(drop(torch.relu(orc._linear(z, w, "linear1"))), w, "linear2"))
        orc._layer_norm(z + ff, w, "norm2").backward(g)
    ms, gib = timed(tstep)
    print(f"torch fp32 autograd (oracle code on the GPU) [1,4,256,{H},{W}]: fwd+bwd {ms:.2f} ms/step, peak {gib:.2f} GiB", flush=True)
