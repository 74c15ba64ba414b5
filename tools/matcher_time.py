"""Prediction-to-ground-truth matching at config 4's size (Q 128, K 124, 4 layers, B 1, pred_masks [128, 16, 64, 64]) for M in {8, 32, 96}:
`axial_vs_amd.match_layers` (one library call for all layers, indices stay on the device) against the only way to do this without it: the
reference's op sequence written with torch on the GPU (softmax over the queries, void-pixel multiply, einsum, class softmax + gather) plus
`C.cpu()` and scipy.optimize.linear_sum_assignment, once per layer.  Also the library's per-stage times (device events between its
launches) and the similarity kernel's achieved bytes / s: the bytes the algorithm needs (every layer's logits once, the targets once per
layer, the partial sums written and read back) over the stage time, against the 8 TB/s HBM figure.

    python tools/matcher_time.py [--steps 2000] [--rounds 5] [--dtype float32|float16]
"""
import argparse
import ctypes
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402
from scipy.optimize import linear_sum_assignment  # noqa: E402

import axial_vs_amd as ax  # noqa: E402
from axial_vs_amd import _lib  # noqa: E402

Q, K, LAYERS, T, H, W = 128, 124, 4, 16, 64, 64
HBM = 8.0e12


def torch_path(layers, targets, masking=True):
    """the matcher's arithmetic as stock torch ops on the GPU, the cost matrix copied to the host (one synchronisation per video per layer)
    and solved by SciPy there"""
    results = []
    for layer in layers:
        for b, gt in enumerate(targets):
            class_prob = torch.softmax(layer["pred_logits"][b].float(), dim=-1)
            class_sim = class_prob[:, :-1].index_select(1, gt["labels"])
            prob = torch.softmax(layer["pred_masks"][b].float().reshape(Q, -1), dim=0)
            gt_masks = gt["masks"].reshape(gt["masks"].shape[0], -1).float()
            if masking:
                nonvoid = gt_masks.sum(dim=0) > 0
                prob = prob * nonvoid.float()[None, :]
            overlap = prob @ gt_masks.T
            mean_area = 0.5 * (prob.sum(dim=1)[:, None] + gt_masks.sum(dim=1)[None, :])
            mask_sim = overlap / (mean_area + 1e-5)
            rows, cols = linear_sum_assignment((-(mask_sim * class_sim)).cpu().numpy())
            results.append((rows, cols, mask_sim[rows, cols], class_sim[rows, cols]))
    return results


def window(fn, steps):
    """one timed window: us per call by device events and by the host clock (the window ends in a device synchronise)"""
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps * 1e3, (time.perf_counter() - t0) / steps * 1e6


def alternate(fa, fb, steps_a, steps_b, warmup, rounds):
    """windows of the two paths in turn, `rounds` of each: (median, min, max) of the host-clock and of the device-event time per call"""
    for _ in range(warmup):
        fa()
        fb()
    wa, wb = [], []
    for _ in range(rounds):
        wa.append(window(fa, steps_a))
        wb.append(window(fb, steps_b))
    stat = lambda xs: (sorted(xs)[len(xs) // 2], min(xs), max(xs))
    return [(stat([w[0] for w in ws]), stat([w[1] for w in ws])) for ws in (wa, wb)]


def stage_times(fn, n=20):
    L = _lib.lib()
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipEventCreate.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
    hip.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), ctypes.c_void_p, ctypes.c_void_p]
    nst = L.axvs_profile_stages(None, 0)
    evs = (ctypes.c_void_p * nst)()
    for i in range(nst):
        e = ctypes.c_void_p()
        hip.hipEventCreate(ctypes.byref(e))
        evs[i] = e.value
    L.axvs_profile_stages(evs, nst)
    acc = {}
    for _ in range(n):
        fn()
        torch.cuda.synchronize()
        for i in range(1, L.axvs_profile_stage_count()):
            ms = ctypes.c_float()
            hip.hipEventElapsedTime(ctypes.byref(ms), evs[i - 1], evs[i])
            nm = L.axvs_profile_stage_name(i).decode()
            acc[nm] = acc.get(nm, 0.0) + ms.value * 1e3 / n
    L.axvs_profile_stages(None, 0)
    return acc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000, help="calls of match_layers per timed window (the torch path gets a quarter)")
    ap.add_argument("--rounds", type=int, default=5, help="alternating windows per path")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--dtype", default="float32")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "matcher_time.py measures on the GPU"
    dt = getattr(torch, a.dtype)
    P = T * H * W
    g = torch.Generator().manual_seed(0)
    layers = [{"pred_masks": (torch.randn(1, Q, T, H, W, generator=g) * 3).to(dt).cuda(), "pred_logits": torch.randn(1, Q, K + 1, generator=g).cuda()}
              for _ in range(LAYERS)]
    outputs = dict(layers[-1], aux_outputs=layers[:-1])
    print(f"Q={Q} K={K} layers={LAYERS} B=1 pred_masks [{Q},{T},{H},{W}] {a.dtype}; us per training step's matching: median (min .. max) of {a.rounds} "
          f"alternating windows of {a.steps} / {a.steps // 4} calls")
    for M in (8, 32, 96):
        owner = torch.randint(0, M + M // 4, (T, H, W), generator=g)
        targets = [{"labels": torch.randint(0, K, (M,), generator=g).cuda(), "masks": torch.stack([owner == m for m in range(M)]).cuda()}]
        (new_ev, new_host), (old_ev, old_host) = alternate(lambda: ax.match_layers(outputs, targets), lambda: torch_path(layers, targets),
                                                           a.steps, max(a.steps // 4, 1), a.warmup, a.rounds)
        got, ref = ax.match_layers(outputs, targets), torch_path([layers[-1]] + layers[:-1], targets)
        same = all(torch.equal(gl[0][0][0].cpu(), torch.as_tensor(r[0])) and torch.equal(gl[0][0][1].cpu(), torch.as_tensor(r[1])) for gl, r in zip(got, ref))
        prev = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")
        try:
            ax.match_layers(outputs, targets)          # raises if the call synchronises with the host
        finally:
            torch.cuda.set_sync_debug_mode(prev)
        st = stage_times(lambda: ax.match_layers(outputs, targets))
        ws_part = _lib.lib().axvs_video_matcher_workspace_bytes(LAYERS, 1, Q, M, P) - 2 * LAYERS * Q * 4
        nbytes = LAYERS * (Q * P * layers[0]["pred_masks"].element_size() + M * P) + 2 * ws_part
        sim = st.get("matcher.similarity", float("nan"))
        f = lambda t: f"{t[0]:8.1f} ({t[1]:.1f} .. {t[2]:.1f})"
        print(f"M={M:3d}: match_layers          host clock {f(new_host)} us, device events {f(new_ev)} us, 0 host synchronisations, same indices: {same}")
        print(f"       torch + .cpu() + SciPy host clock {f(old_host)} us, device events {f(old_ev)} us, {LAYERS} host synchronisations")
        print(f"       ratio of the host-clock medians {old_host[0] / new_host[0]:.1f}x (worst window against best: {old_host[1] / new_host[2]:.1f}x)")
        print("        stages: " + "  ".join(f"{k}={v:.1f}us" for k, v in st.items()) +
              f" | similarity kernel: {nbytes / 1e6:.1f} MB needed -> {nbytes / (sim * 1e-6) / 1e12:.2f} TB/s = {nbytes / (sim * 1e-6) / HBM * 100:.0f}% of 8 TB/s")


if __name__ == "__main__":
    main()
