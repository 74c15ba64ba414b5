"""One training step's Tube-Link loss + backward at the ytvis21 cross-clip head's size (L 6 layers, B 1, Q 100, T 9, 128 x 228, K 40,
num_points 12544, oversample 3.0, importance ratio 0.75) for M in {8, 32}: `axial_vs_amd.tube_link_losses` (cost, assignment, selection,
losses and gradients in the library, no host synchronisation) against the reference's op sequence written with torch on the same GPU
(mask2former_video_cc_head.py:519-694: grid_sample for every point_sample, the three cost terms, `.cpu()` + SciPy per (layer, video),
boolean indexing of the matched masks, topk, autograd for the backward).  Reports us per step (host clock and device events), the host
synchronisations of one step (torch.cuda.set_sync_debug_mode), and the bytes a step allocates.

    python tools/tl_loss_time.py [--steps 20] [--rounds 5] [--out profiles/tl_loss_time.md]
    python tools/tl_loss_time.py --library-only --steps 20      # the library path alone, for a kernel trace of its own
"""
import argparse
import os
import sys
import warnings

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import axial_vs_amd as ax  # noqa: E402
from matcher_time import alternate, window  # noqa: E402

L, B, Q, T, H, W, K = 6, 1, 100, 9, 128, 228, 40
P, OVER, RATIO = 12544, 3.0, 0.75
COST_W = LOSS_W = (2.0, 5.0, 5.0)


def point_sample(img, pts):
    return F.grid_sample(img, 2.0 * pts.unsqueeze(2) - 1.0, align_corners=False).squeeze(3)


def torch_loss(cls_all, masks_all, labels, gt, cw):
    """the reference's loss() as stock torch ops in fp32, with its host round trips"""
    from scipy.optimize import linear_sum_assignment
    S, k = int(P * OVER), int(RATIO * P)
    total = 0.0
    for cls, mp in zip(cls_all, masks_all):
        lab = torch.full((B, Q), K, dtype=torch.int64, device="cuda")
        weights = torch.zeros(B, Q, device="cuda")
        tgts = []
        for b in range(B):
            gl = gt[b].flatten(1, 2)
            lp = mp[b].transpose(1, 0).flatten(1, 2)
            pc = torch.rand((1, P, 2), device="cuda")
            x = point_sample(lp.unsqueeze(1), pc.repeat(Q, 1, 1)).squeeze(1)
            g = point_sample(gl.unsqueeze(1).float(), pc.repeat(gl.shape[0], 1, 1)).squeeze(1)
            c_cls = -cls[b].softmax(-1)[:, labels[b]]
            pos = F.binary_cross_entropy_with_logits(x, torch.ones_like(x), reduction="none")
            neg = F.binary_cross_entropy_with_logits(x, torch.zeros_like(x), reduction="none")
            c_mask = (torch.einsum("nc,mc->nm", pos, g) + torch.einsum("nc,mc->nm", neg, 1 - g)) / P
            s = x.sigmoid()
            c_dice = 1 - (2 * torch.einsum("nc,mc->nm", s, g) + 1.0) / (s.sum(-1)[:, None] + g.sum(-1)[None, :] + 1.0)
            cost = (COST_W[0] * c_cls + COST_W[1] * c_mask + COST_W[2] * c_dice).detach().cpu()
            r, c = linear_sum_assignment(cost)
            r, c = torch.from_numpy(r).cuda(), torch.from_numpy(c).cuda()
            lab[b, r] = labels[b][c]
            weights[b, r] = 1.0
            tgts.append(gl[c])
        lab = lab.flatten()
        loss_cls = LOSS_W[0] * (F.cross_entropy(cls.flatten(0, 1), lab, weight=cw, reduction="none").sum() / cw[lab].sum())
        ntm = max(cls.new_tensor([float(sum(t.shape[0] for t in tgts))]), 1)
        mt = torch.cat(tgts)
        mpm = mp.transpose(2, 1).flatten(2, 3)[weights > 0]
        with torch.no_grad():
            cand = torch.rand(mpm.shape[0], S, 2, device="cuda")
            unc = -point_sample(mpm.unsqueeze(1), cand).abs()
            idx = torch.topk(unc[:, 0, :], k=k, dim=1)[1]
            idx = idx + S * torch.arange(mpm.shape[0], dtype=torch.long, device="cuda")[:, None]
            pts = torch.cat((cand.view(-1, 2)[idx.view(-1)].view(mpm.shape[0], k, 2), torch.rand(mpm.shape[0], P - k, 2, device="cuda")), 1)
            t = point_sample(mt.unsqueeze(1).float(), pts).squeeze(1)
        x = point_sample(mpm.unsqueeze(1), pts).squeeze(1)
        s = x.sigmoid()
        loss_dice = LOSS_W[2] * ((1 - (2 * (s * t).sum(1) + 1.0) / (s.sum(1) + t.sum(1) + 1.0)).sum() / ntm)
        loss_mask = LOSS_W[1] * (F.binary_cross_entropy_with_logits(x.reshape(-1), t.reshape(-1), reduction="none").sum() / (ntm * P))
        total = total + loss_cls + loss_mask.sum() + loss_dice.sum()
    return total


def syncs(fn):
    """host synchronisations of one call, counted by torch's sync debug mode"""
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    return sum("synchroniz" in str(w.message) for w in rec)


def peak(fn, clear):
    clear()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20, help="steps of the library path per timed window (the torch path gets half)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--library-only", action="store_true")
    ap.add_argument("--out", default=None, help="also write the report there")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tl_loss_time.py measures on the GPU"
    g = torch.Generator().manual_seed(0)
    cls = [torch.randn(B, Q, K + 1, generator=g).cuda().requires_grad_(True) for _ in range(L)]
    masks = [(torch.randn(B, T, Q, H, W, generator=g) * 3).cuda().requires_grad_(True) for _ in range(L)]
    leaves = cls + masks
    cw = torch.tensor([1.0] * K + [0.1]).cuda()
    lines = [f"L={L} B={B} Q={Q} T={T} {H}x{W} K={K} num_points={P} oversample={OVER} importance ratio={RATIO}, mask_preds fp32 [{B},{T},{Q},{H},{W}] per layer; "
             f"{torch.cuda.get_device_name(0)}, torch {torch.__version__}",
             f"us per step (loss forward + backward): median (min .. max) of {a.rounds} alternating windows of {a.steps} / {max(a.steps // 2, 1)} steps", ""]

    def clear():
        for v in leaves:
            v.grad = None

    for M in (8, 32):
        owner = torch.randint(0, M + M // 4, (T, H, W), generator=g)
        labels = [torch.randint(0, K, (M,), generator=g).cuda()]
        gt = [torch.stack([owner == m for m in range(M)]).cuda()]

        def new():
            clear()
            sum(ax.tube_link_losses(cls, masks, labels, gt, num_classes=K, class_weight=cw, num_points=P, oversample_ratio=OVER,
                                    importance_sample_ratio=RATIO).values()).backward()

        def old():
            clear()
            torch_loss(cls, masks, labels, gt, cw).backward()

        if a.library_only:
            for _ in range(a.warmup):
                new()
            ev, host = window(new, a.steps)
            print(f"M={M}: library {host:.1f} us host clock, {ev:.1f} us device events per step")
            continue
        (new_ev, new_host), (old_ev, old_host) = alternate(new, old, a.steps, max(a.steps // 2, 1), a.warmup, a.rounds)
        sn, so = syncs(new), syncs(old)
        mem_new, mem_old = peak(new, clear), peak(old, clear)
        ln = float(sum(ax.tube_link_losses(cls, masks, labels, gt, num_classes=K, class_weight=cw, num_points=P, oversample_ratio=OVER,
                                           importance_sample_ratio=RATIO, generator=torch.Generator(device="cuda").manual_seed(1)).values()))
        torch.manual_seed(1)
        lo = float(torch_loss(cls, masks, labels, gt, cw))
        f = lambda t: f"{t[0]:9.1f} ({t[1]:.1f} .. {t[2]:.1f})"
        lines += [f"M={M:3d}: library              host clock {f(new_host)} us, device events {f(new_ev)} us, {sn} host synchronisations, {mem_new:7.1f} MB allocated over a step",
                  f"       torch + .cpu() + SciPy host clock {f(old_host)} us, device events {f(old_ev)} us, {so} host synchronisations (L*B + L = {L * B + L} named in the "
                  f"reference's text), {mem_old:7.1f} MB allocated over a step",
                  f"       ratio of the host-clock medians {old_host[0] / new_host[0]:.2f}x (worst library window against best torch window: {old_host[1] / new_host[2]:.2f}x), "
                  f"memory {mem_old / mem_new:.1f}x; total loss under the same generator seed {ln:.6f} / {lo:.6f}", ""]
    text = "\n".join(lines)
    print(text)
    if a.out and not a.library_only:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
