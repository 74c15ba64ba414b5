"""One training step's matching + set criterion + backward at config 4's size (N 128, K 124, 4 layers, B 1, pred_masks [128, 16, 64, 64]) for
M in {8, 32, 96}: `axial_vs_amd.MaXTronCCSetCriterion` (matcher, losses and gradients in the library, no host synchronisation) against the
only way to do this without it: the reference's op sequence written with torch on the GPU (tools/matcher_time.torch_path for its matcher:
torch ops + `.cpu()` + SciPy; then the scatter into a zero tensor shaped like pred_masks, the softmax for the void IoU, softmax + log-softmax
for the mask losses, autograd for the backward).  Also torch.cuda.max_memory_allocated over a step for both paths, and the achieved bytes / s
of the criterion's forward and backward calls (matcher excluded) against the bytes the algorithm needs: pred_masks once forward, once
plus one write backward, the targets once per layer each way.

    python tools/criterion_time.py [--steps 200] [--rounds 5] [--out profiles/criterion_time.md]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import axial_vs_amd as ax  # noqa: E402
from axial_vs_amd import criterion as axc  # noqa: E402
from matcher_time import HBM, H, K, LAYERS, Q, T, W, alternate, torch_path, window  # noqa: E402


def torch_criterion(layers, targets, masking=True):
    """the reference's shared-matching criterion (cc_criterion.py:338-453) as stock torch ops in fp32; layers[0] is the final prediction"""
    with torch.no_grad():
        rows, cols, dice, cls = torch_path(layers[:1], targets, masking)[0]
    rows, cols = torch.as_tensor(rows, device="cuda"), torch.as_tensor(cols, device="cuda")
    src = layers[0]["pred_masks"].detach()
    with torch.no_grad():
        tm = torch.zeros_like(src)
        tm[0, rows] = targets[0]["masks"][cols].to(tm)
        w_mask = torch.zeros(src.shape[:2], device="cuda")
        w_mask[0, rows] = cls.clamp(min=1e-5)
        void = tm.sum(1) < 1
        label = torch.full(src.shape[:2], K, dtype=torch.int64, device="cuda")
        label[0, rows] = targets[0]["labels"][cols]
        prob = src.softmax(1).flatten(2)
        w_cls = torch.einsum("bnl,bl->bn", prob, void.flatten(1).to(prob)) / (prob.sum(-1) + 1e-5)
        w_cls[0, rows] = dice
        w_cls = w_cls.clamp(min=1e-5)
        t, v = tm.flatten(2), void.flatten(1)
    total = 0.0
    for o in layers:
        x = o["pred_masks"].flatten(2)
        ce = F.cross_entropy(x, t, reduction="none")
        q = x.softmax(1)
        if masking:
            ce = ce.masked_fill(v, 0)
            q = q.masked_fill(v.unsqueeze(1), 0)
        loss_mask = (ce.sum(-1) / (ce != 0).to(ce).sum(-1).clamp(min=1.0)).mean()
        dl = (1.0 - (2 * (q * t).sum(-1) + 1.0) / (q.sum(-1) + t.sum(-1) + 1.0)) * w_mask
        loss_dice = (dl.sum(1) * 0.75 / x.shape[1]).mean()
        lg = o["pred_logits"].transpose(1, 2)
        gt = F.one_hot(label, K + 1).transpose(1, 2).to(lg)
        fl = F.cross_entropy(lg, gt, reduction="none") * (0.75 * (1.0 - gt[:, -1]) + 0.25 * gt[:, -1]) * w_cls
        loss_ce = (fl.sum(-1) / (fl != 0).to(fl).sum(-1).clamp(min=1.0)).mean()
        total = total + loss_ce + loss_mask + loss_dice
    return total


def peak(fn, clear):
    """bytes a step allocates above what is live before it (the previous step's gradients released first, as optimizer.zero_grad() does)"""
    clear()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200, help="steps of the library path per timed window (the torch path gets a quarter)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the report there")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "criterion_time.py measures on the GPU"
    P = T * H * W
    g = torch.Generator().manual_seed(0)
    layers = [{"pred_masks": (torch.randn(1, Q, T, H, W, generator=g) * 3).cuda().requires_grad_(True),
               "pred_logits": torch.randn(1, Q, K + 1, generator=g).cuda().requires_grad_(True)} for _ in range(LAYERS)]
    outputs = dict(layers[0], aux_outputs=layers[1:])
    leaves = [v for o in layers for v in o.values()]
    crit = ax.MaXTronCCSetCriterion(K, ax.VideoHungarianMatcher(True), {}, 0.1, ["labels", "masks"], True)
    lines = [f"N={Q} K={K} layers={LAYERS} B=1 pred_masks [{Q},{T},{H},{W}] fp32, shared final matching, masking_void_pixel; "
             f"{torch.cuda.get_device_name(0)}, torch {torch.__version__}",
             f"us per step (matcher + criterion forward + backward): median (min .. max) of {a.rounds} alternating windows of {a.steps} / {max(a.steps // 4, 1)} steps", ""]

    def clear():
        for v in leaves:
            v.grad = None

    for M in (8, 32, 96):
        owner = torch.randint(0, M + M // 4, (T, H, W), generator=g)
        targets = [{"labels": torch.randint(0, K, (M,), generator=g).cuda(), "masks": torch.stack([owner == m for m in range(M)]).cuda()}]

        def new():
            clear()
            sum(crit(outputs, targets).values()).backward()

        def old():
            clear()
            torch_criterion(layers, targets).backward()

        (new_ev, new_host), (old_ev, old_host) = alternate(new, old, a.steps, max(a.steps // 4, 1), a.warmup, a.rounds)
        new()
        gn = [v.grad.clone() for v in leaves]
        ln = float(sum(crit(outputs, targets).values()))
        old()
        agree = max(float((x - v.grad).abs().max() / v.grad.abs().max()) for x, v in zip(gn, leaves))
        lo = float(torch_criterion(layers, targets))
        mem_new, mem_old = peak(new, clear), peak(old, clear)
        # the criterion's two calls alone: the matching done once outside the window
        losses = axc._criterion(outputs, targets, K, True, True)
        gl = torch.ones_like(losses)
        calls = [lambda: axc._criterion(outputs, targets, K, True, True), lambda: ax.match_layers({k: v.detach() for k, v in layers[0].items()}, targets),
                 lambda: torch.autograd.grad(losses, leaves, gl, retain_graph=True)]
        for c in calls:
            for _ in range(a.warmup):
                c()
        (fwd_ev, _), (mt_ev, _), (bwd_ev, _) = [window(c, a.steps) for c in calls]
        fb = LAYERS * (Q * P * 4 + M * P)
        bb = LAYERS * (2 * Q * P * 4 + M * P)
        f = lambda t: f"{t[0]:8.1f} ({t[1]:.1f} .. {t[2]:.1f})"
        lines += [f"M={M:3d}: library              host clock {f(new_host)} us, device events {f(new_ev)} us, peak memory over a step {mem_new:7.1f} MB, 0 host synchronisations",
                  f"       torch + .cpu() + SciPy host clock {f(old_host)} us, device events {f(old_ev)} us, peak memory over a step {mem_old:7.1f} MB",
                  f"       ratio of the host-clock medians {old_host[0] / new_host[0]:.2f}x (worst library window against best torch window: {old_host[1] / new_host[2]:.2f}x), "
                  f"memory {mem_old / mem_new:.1f}x; total loss {ln:.6f} / {lo:.6f}, largest gradient difference {agree:.1e} of the largest entry",
                  f"       criterion forward (one matching of the final layer, {mt_ev:.1f} us, included) {fwd_ev:.1f} us: {fb / 1e6:.1f} MB needed -> "
                  f"{fb / ((fwd_ev - mt_ev) * 1e-6) / 1e12:.2f} TB/s = {fb / ((fwd_ev - mt_ev) * 1e-6) / HBM * 100:.0f}% of 8 TB/s without it; "
                  f"backward {bwd_ev:.1f} us: {bb / 1e6:.1f} MB -> {bb / (bwd_ev * 1e-6) / 1e12:.2f} TB/s = {bb / (bwd_ev * 1e-6) / HBM * 100:.0f}%", ""]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
