"""The two sampled pixel losses of one training step at the within-clip R50 config's size (7 predictions, N 128, T 2, 193 x 337,
pixel_feature C 128, 124 classes, k 4096; B in {1, 2}, M in {8, 32}): `axial_vs_amd.criterion._sampled_losses` forward + backward (the
matching is done once outside the window: it belongs to the `labels` / `masks` call) against the reference's op sequence for the same
two losses (wc_criterion.py:62-142, :341-415) written with stock torch ops in fp32 on the same GPU, on the same noise.  Reports device
time per step, bytes allocated over a step, kernel launches and the kernel with the largest share (torch.profiler, a run of its own),
and runs one library step under torch.cuda.set_sync_debug_mode("error"): a host synchronisation would raise.

    python tools/pixel_losses_time.py [--steps 20] [--rounds 5] [--out profiles/pixel_losses_time.md]
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
from matcher_time import alternate  # noqa: E402

LAYERS, N, T, H, W, C, K, KS = 7, 128, 2, 193, 337, 128, 124, 4096
TEMPS = (1.8, 2.4)
MFMA_F32_PEAK = 157.3e12


def torch_losses(layers, targets, rows, cols, noise, keep=None):
    """the reference's shared-matching op sequence for `pixels` and `aux_semantic`, fp32 torch ops; rows / cols: per video, on the GPU"""
    B, P = len(targets), T * H * W
    with torch.no_grad():
        tm = torch.zeros(B, N, P, device="cuda")
        for b in range(B):
            tm[b, rows[b]] = targets[b]["masks"][cols[b]].flatten(1).float()
        void = tm.sum(1) < 1
        area = tm.sum(2)
        inv = P / torch.einsum("bnp,bn->bp", tm, area).clamp(min=1.0)
        sem = torch.stack([t["semantic_masks"].reshape(P) for t in targets]).clone()
        sem[sem == -1] = K

    def sample(u, temp, k):
        logits = torch.log(inv) * temp
        logits = logits + void.to(logits) * -99999.0
        idx = torch.topk(logits + -torch.log(-torch.log(u)), k)[1]
        if keep is not None:
            keep.append(idx.sort(-1).values)
        return idx

    def mean(loss):
        return (loss.sum(-1) / (loss != 0).to(loss).sum(-1).clamp(min=1.0)).mean()
    total = 0.0
    for l, o in enumerate(layers):
        idx = sample(noise[0][l], TEMPS[0], KS)
        g = torch.gather(tm, 2, idx.unsqueeze(1).expand(-1, N, -1))
        gs = torch.einsum("bnk,bnj->bkj", g, g)
        gs = gs / gs.sum(1, keepdim=True).clamp(min=1.0)
        f = torch.gather(o["pixel_feature"].flatten(2), 2, idx.unsqueeze(1).expand(-1, C, -1))
        s = torch.einsum("bck,bcj->bkj", f, f) / 0.3
        total = total + mean(F.cross_entropy(s, gs, reduction="none"))
        if l == 0:
            idx = sample(noise[1], TEMPS[1], KS)
            x = torch.gather(o["aux_semantic_pred"].flatten(2), 2, idx.unsqueeze(1).expand(-1, K, -1))
            tg = torch.gather(sem, 1, idx)
            total = total + mean(F.cross_entropy(x, tg, ignore_index=K, reduction="none") * (tg != K).to(x))
    return total


def peak(fn, clear):
    clear()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 1e6


def kernels(fn, clear):
    """(launches, [(name, total us)] by time) of one step, from torch.profiler; None when the profiler gives no kernel records"""
    from torch.profiler import ProfilerActivity, profile
    clear()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    ev = [e for e in prof.events() if str(e.device_type).endswith("CUDA")]
    if not ev:
        return None
    by = {}
    for e in ev:
        by[e.name] = by.get(e.name, 0.0) + e.device_time
    return len(ev), sorted(by.items(), key=lambda kv: -kv[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "pixel_losses_time.py measures on the GPU"
    P = T * H * W
    g = torch.Generator().manual_seed(0)
    torch.manual_seed(0)
    lines = [f"layers={LAYERS} N={N} T={T} {H}x{W} (P={P}) C={C} classes={K} k={KS}, shared final matching; {torch.cuda.get_device_name(0)}, torch {torch.__version__}",
             f"us per step (the two losses, forward + backward, matching excluded): median (min .. max) of {a.rounds} alternating windows of {a.steps} steps",
             f"contractions of the instance-discrimination forward: 2 k^2 (C + 16 ceil(pairs / 16)) FLOP per prediction and video", ""]
    for B, M in ((1, 8), (1, 32), (2, 8), (2, 32)):
        layers = []
        for l in range(LAYERS):
            o = {"pred_masks": (torch.randn(B, N, T, H, W, generator=g) * 3).cuda(), "pred_logits": torch.randn(B, N, K + 1, generator=g).cuda(),
                 "pixel_feature": (torch.randn(B, C, T, H, W, generator=g) * 0.3).cuda().requires_grad_(True)}
            if l == 0:
                o["aux_semantic_pred"] = torch.randn(B, K, T, H, W, generator=g).cuda().requires_grad_(True)
            layers.append(o)
        outputs = dict(layers[0], aux_outputs=layers[1:])
        leaves = [o["pixel_feature"] for o in layers] + [layers[0]["aux_semantic_pred"]]
        targets = []
        for b in range(B):
            owner = torch.randint(0, M + M // 4, (T, H, W), generator=g)
            targets.append({"labels": torch.randint(0, K, (M,), generator=g).cuda(), "masks": torch.stack([owner == m for m in range(M)]).cuda(),
                            "semantic_masks": torch.randint(-1, K, (T, H, W), generator=g).cuda()})
        st = axc._match_step(outputs, targets, K, True, True)
        pairs = ax.match_layers({k: v.detach() for k, v in layers[0].items()}, targets)[0][0]
        rows, cols = [p[0] for p in pairs], [p[1] for p in pairs]
        noise = ax.draw_sampling_noise(LAYERS, B, P, True, True, "cuda")

        def clear():
            for v in leaves:
                v.grad = None

        def new():
            clear()
            res, _ = axc._sampled_losses(st, targets, K, ("pixels", "aux_semantic"), TEMPS, (KS, KS), noise, None, False)
            (res["pixels"].sum() + res["aux_semantic"].sum()).backward()

        def old():
            clear()
            torch_losses(layers, targets, rows, cols, noise).backward()

        (new_ev, _), (old_ev, _) = alternate(new, old, a.steps, a.steps, a.warmup, a.rounds)
        res, _ = axc._sampled_losses(st, targets, K, ("pixels", "aux_semantic"), TEMPS, (KS, KS), noise, None, False)
        kept = []
        ln, lo = float(res["pixels"].sum() + res["aux_semantic"].sum()), float(torch_losses(layers, targets, rows, cols, noise, kept))
        _, smp = axc._sampled_losses(st, targets, K, ("pixels", "aux_semantic"), TEMPS, (KS, KS), noise, None, True)
        mine = [smp["pixels"][0], smp["aux_semantic"]] + [smp["pixels"][l] for l in range(1, LAYERS)]      # torch_losses' call order
        swapped = sum(int((a.long() != b).any(-1).sum()) for a, b in zip(mine, kept))
        new()
        gn = [v.grad.clone() for v in leaves]
        old()
        agree = max(float((x - v.grad).abs().max() / v.grad.abs().max()) for x, v in zip(gn, leaves))
        mem_new, mem_old = peak(new, clear), peak(old, clear)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            new()
            syncs = "0 host synchronisations (a step under set_sync_debug_mode('error') raised nothing)"
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        f = lambda t: f"{t[0]:9.1f} ({t[1]:.1f} .. {t[2]:.1f})"
        lines += [f"B={B} M={M:2d}: library device events {f(new_ev)} us, {mem_new:8.1f} MB allocated over a step, {syncs}",
                  f"           torch   device events {f(old_ev)} us, {mem_old:8.1f} MB allocated over a step",
                  f"           torch / library {old_ev[0] / new_ev[0]:.2f}x in time, {mem_old / mem_new:.1f}x in memory; total loss {ln:.6f} / {lo:.6f}, "
                  f"largest gradient difference {agree:.1e} of the largest entry; "
                  f"{swapped} of {(LAYERS + 1) * B} sample sets differ from torch's (fp32 keys within a rounding of each other at the k-th place: unscreened noise)"]
        try:
            kn, ko = kernels(new, clear), kernels(old, clear)
        except Exception as e:      # the profiler is optional equipment
            kn = ko = None
            lines.append(f"           kernel records: not measured ({type(e).__name__})")
        if kn and ko:
            flop = 2.0 * KS * KS * (C + 16 * ((min(N, M) + 15) // 16)) * LAYERS * B
            top = kn[1][0]
            lines += [f"           launches per step: library {kn[0]}, torch {ko[0]}",
                      f"           library kernels by time: " + ", ".join(f"{n.split('(')[0][-40:]} {t:.0f} us" for n, t in kn[1][:4])]
            fwd = [t for n, t in kn[1] if "px_insdis_fwd" in n]
            if fwd:
                lines.append(f"           px_insdis_fwd_kernel: {flop / 1e9:.1f} GFLOP in {fwd[0]:.0f} us = {flop / (fwd[0] * 1e-6) / 1e12:.1f} TFLOP/s = "
                             f"{flop / (fwd[0] * 1e-6) / MFMA_F32_PEAK * 100:.0f}% of the f32 MFMA peak; {KS * KS * LAYERS * B / 1e6:.0f} M exponentials")
            lines.append(f"           largest share: {top[0].split('(')[0][-40:]} ({top[1] / sum(t for _, t in kn[1]) * 100:.0f}% of the kernel time)")
        lines.append("")
    # the whole criterion as the within-clip model builds it, on the last configuration: matcher, four losses, backward
    crit = ax.MaXTronWCSetCriterion(K, ax.VideoHungarianMatcher(), {}, 0.1, ["labels", "masks", "pixels", "aux_semantic"], True, process_semantic=True,
                                    pixel_insdis_temperature=TEMPS[0], aux_semantic_temperature=TEMPS[1])
    for o in layers:
        o["pred_masks"].requires_grad_(True)
        o["pred_logits"].requires_grad_(True)

    def whole():
        clear()
        sum(crit(outputs, targets).values()).backward()
    whole()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        whole()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    (ev, _), _ = alternate(whole, whole, a.steps, 1, a.warmup, a.rounds)
    lines += [f"MaXTronWCSetCriterion(124, matcher, {{}}, 0.1, [labels, masks, pixels, aux_semantic], True, process_semantic=True, 1.8 / 2.4) at B={B} M={M}: "
              f"matcher + four losses + backward {ev[0]:.1f} ({ev[1]:.1f} .. {ev[2]:.1f}) us per step by device events; a step under "
              f"set_sync_debug_mode('error') raised nothing: 0 host synchronisations", ""]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
