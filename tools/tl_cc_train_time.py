"""Training step (forward + backward) of the Tube-Link cross-clip head (TubeLinkCrossClipHead in train()) at the ytvis21 cross-clip
config's size: B 1, 3 clips of 3 frames, Q 100, 4 layers, K1 41, Cm 256, mask features 128 x 228 and 96 x 168 (training short side
512 / 384).  Median ms per step over n steps (default 20) and peak memory, for the library's heads tier (chain + axvs_tl_heads_train_*)
and for the torch heads it replaced: post_norm, activation_proj + softmax, cls_embed, the mask_embed MLP and the per-clip einsum as the
module's torch layers around the chain's training tier (cc_layers_train).  The mask features carry no gradient (the frozen decoder)."""
import os, statistics, sys, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import axial_vs_amd as ax
from axial_vs_amd.cc_training import cc_layers_train

n = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 20
B, Tc, fpc, Q, nl, K, Cm = 1, 3, 3, 100, 4, 40, 256


def timed(step):
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    times = []
    for _ in range(n):
        t0 = time.perf_counter()
        step()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return statistics.median(times) * 1e3, torch.cuda.max_memory_allocated() / 2 ** 30


torch.manual_seed(0)
mod = ax.TubeLinkCrossClipHead(num_classes=K, out_channels=Cm, num_cc_layers=nl, trajectory_drop_out=0.0, drop_path_prob=0.0).cuda().train()
cq = torch.randn(B, Tc, Q, 256, device="cuda").requires_grad_(True)


def torch_heads(mf):       # TLCC:761-797 per layer and clip, as the reference's torch modules (the module's train() mode before the tier)
    queries = cc_layers_train(mod, cq.permute(0, 2, 1, 3).contiguous(), nl, mod.atrous_rates, 0.0, 0.0)
    cls_all, mask_all = [], []
    for i in range(nl):
        xn = mod.transformer_decoder.post_norm(queries[i]).permute(0, 2, 1, 3)
        act = torch.softmax(mod.activation_proj(xn), dim=1)
        cls_all.append(mod.cls_embed((xn * act).sum(dim=1)))
        me = mod.mask_embed(xn)
        mask_all.append(torch.cat([torch.einsum("bqc,btchw->btqhw", me[:, c], mf[:, fpc * c:fpc * (c + 1)]) for c in range(Tc)], dim=1))
    return cls_all, mask_all


for h, w in ((128, 228), (96, 168)):
    mf = torch.nn.functional.normalize(torch.randn(B, Tc * fpc, Cm, h, w, device="cuda"), dim=2)
    for label, fwd in (("heads tier", lambda: mod(cq, mf)), ("torch heads", lambda: torch_heads(mf))):
        def step():
            cls, masks = fwd()
            (sum(c.sum() for c in cls) + sum(x.square().sum() for x in masks) * 1e-3).backward()
        ms, gib = timed(step)
        print(f"{h} x {w}, {label}: chain + heads fwd+bwd {ms:.3f} ms/step (median of {n}), peak {gib:.2f} GiB", flush=True)
        mod.zero_grad(set_to_none=True)
        cq.grad = None
