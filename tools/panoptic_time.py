"""Video panoptic post-processing: `axial_vs_amd.video_panoptic_inference` against the only way to do it without the library, the
reference's op sequence (maxtron_cc_model.py:442-571: two `F.interpolate`, the softmax over the slots at full resolution, the
threshold, `argsort`, the Python loop over the slots with its `.item()` synchronisations, the relabelling loop) written with torch on
the same GPU (tests/panoptic_cases.post_process + merge, nothing counted).

Sizes: N 128, K 124, low resolution 180 x 320 -> 720 x 1280 with T 2 and T 8, and a Cityscapes-VPS-like N 128, K 19, T 2,
256 x 512 -> 1024 x 2048; each with scale_factor 1 (crop only) and 0.7 (the crop of the resized logits resized again to 1 / 0.7 its
size).  Per size: hipEvent times (median, min .. max over the repeats, every call timed on its own), the ratio, the peak memory a call
allocates above its inputs, the pixels at which the two maps differ (the inputs are not screened: a score within the fp32 error of a
threshold may fall either way), and the pixel pass's achieved bandwidth over the bytes it has to move: the low-resolution logits once
and 4 bytes per output pixel (the kernel's time comes from torch.profiler's device trace).

    python tools/panoptic_time.py [--reps 20] [--out profiles/panoptic_time.md]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import axial_vs_amd as ax  # noqa: E402
from axial_vs_amd import modules  # noqa: E402
import panoptic_cases as pc  # noqa: E402

HBM = 8e12
SETTING = pc.SETTINGS[0]          # the shipped VIPSeg thresholds: pixel 0.4, overlap 0.8, class 0.7 / 0.5, reorder 1 / 1
SIZES = [("N128 T2 180x320 -> 720x1280", (128, 2, 180, 320, 720, 1280, 124)), ("N128 T8 180x320 -> 720x1280", (128, 8, 180, 320, 720, 1280, 124)),
         ("Cityscapes-VPS-like N128 T2 256x512 -> 1024x2048", (128, 2, 256, 512, 1024, 2048, 19))]


def geometry(c, sf):
    N, T, h, w, H, W, K = c
    if sf >= 1:
        return pc.SimpleNamespace(ac=W % 2 == 1, image_h=H, image_w=W, sf=sf, scaled_h=H, scaled_w=W, height=H, width=W)
    sh, sw = H - 16, W - 16              # the padded image minus its padding
    return pc.SimpleNamespace(ac=W % 2 == 1, image_h=H, image_w=W, sf=sf, scaled_h=sh, scaled_w=sw, height=round(sh / sf), width=round(sw / sf))


def timed(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def peak(fn):
    modules._workspaces.clear()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 1e6, out


def kernel_us(fn, name):
    """median device time of the kernels whose name contains `name` over 5 calls, from torch.profiler's device trace; None without one"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(5):
                fn()
            torch.cuda.synchronize()
        us = [e.device_time_total / max(e.count, 1) for e in prof.key_averages() if name in e.key]
        return us[0] if us else None
    except Exception as e:          # no device trace on this installation: the report says so
        print(f"(torch.profiler gave no device trace: {e})", file=sys.stderr)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20, help="timed calls of the library path (the torch path gets a quarter, at least 3)")
    ap.add_argument("--out", default=None, help="also write the report there")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "panoptic_time.py measures on the GPU"
    thr, ov, ct, cs, rc, rm = SETTING
    lines = [f"{torch.cuda.get_device_name(0)}, torch {torch.__version__}; thresholds {SETTING}; mask logits fp32",
             f"ms per call by device events: median (min .. max) of {a.reps} / {max(a.reps // 4, 3)} calls, each timed on its own", ""]
    table = ["| size | scale_factor | library | torch composition | ratio | peak memory |", "|---|---|---|---|---|---|"]
    for name, c in SIZES:
        N, T, h, w, H, W, K = c
        mp, cls, emb = (x.cuda() for x in pc.make_inputs(c, 7))
        things, stuff = pc.ids_of(K)
        post = ax.VideoPanopticPostProcessor(things, stuff, pc.LABEL_DIVISOR, ct, cs, thr, ov, rc, rm)
        for sf in (1.0, 0.7):
            g = geometry(c, sf)
            args = (g.ac, g.image_h, g.image_w, g.sf, g.scaled_h, g.scaled_w, g.height, g.width)
            new = lambda: post(cls, mp, emb, *args)
            old = lambda: pc.merge(cls, pc.post_process(mp, g), emb, SETTING, things, stuff, stats=False)[:2]
            tn, to = timed(new, a.reps), timed(old, max(a.reps // 4, 3), warmup=1)
            mem_new, (seg, d) = peak(new)
            mem_old, (ref, dr) = peak(old)
            P = seg.numel()
            diff = int((seg != ref).sum())
            us = kernel_us(lambda: post(cls, mp, emb, *args, return_tables=True), "panoptic_pixel_kernel")
            need = mp.numel() * 4 + P * 4
            bw = f"pixel pass {us:.1f} us for {need / 1e6:.1f} MB: {need / (us * 1e-6) / 1e12:.2f} TB/s = {need / (us * 1e-6) / HBM * 100:.0f}% of 8 TB/s" if us else \
                 "pixel pass: no device trace"
            f = lambda t: f"{t[0]:9.3f} ({t[1]:.3f} .. {t[2]:.3f})"
            lines += [f"{name}, scale_factor {sf}: map [{T}, {seg.shape[1]}, {seg.shape[2]}], {len(d)} thing categories",
                      f"    library (one synchronisation, for the dict) {f(tn)} ms, peak memory above the inputs {mem_new:9.1f} MB (the map itself: {P * 4 / 1e6:.1f} MB)",
                      f"    torch composition                          {f(to)} ms, peak memory above the inputs {mem_old:9.1f} MB",
                      f"    ratio of the medians {to[0] / tn[0]:.1f}x (slowest library call against fastest torch call: {to[1] / tn[2]:.1f}x), memory {mem_old / mem_new:.0f}x; "
                      f"{diff} of {P} pixels differ, dict keys equal: {list(d) == list(dr)}",
                      f"    {bw}", ""]
            table.append(f"| {name} | {sf} | {tn[0]:.2f} ms | {to[0]:.1f} ms | {to[0] / tn[0]:.0f}x | {mem_new:.0f} MB against {mem_old:.0f} MB |")
            del seg, ref
    text = "\n".join(lines + table)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
