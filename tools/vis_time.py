"""Video instance post-processing: `axial_vs_amd.video_instance_inference` against the only way to do it without the library, the
reference's op sequence written with torch on the same GPU: the whole-video `F.interpolate` to batch_input_shape
(mask2former_video_cc_head.py:1026-1034), then per frame the crop, `topk`, the gather, the second `F.interpolate` to ori_shape, `> 0`,
the mean sigmoid, `mask2bbox` with its Python loop and two `torch.where` synchronisations per mask (maskformer_fusion_head.py:426-462,
mmdet/core/mask/utils.py:68-89), the argsort, `[:30]`, `bbox2result` and thirty `.cpu().numpy()` mask copies
(mask2former_vis_video.py:184-199).  The restated sequence is the yardstick; the library is never its own baseline.

Inputs: 60 of the 100 queries have all-negative logits (the library skips a query in every tile where its box holds no positive value,
the torch composition does not care), except in the "no empty query" line, where every query is noise that is positive at half of the
pixels: the two ends of what real masks give.

Sizes: the YouTube-VIS test size (Q 100, C 40, 96 x 160 -> 384 x 640, crop 360 x 640 -> 720 x 1280) at T 5 and T 36, and an OVIS-like
one (Q 100, C 25, 90 x 160 -> 360 x 640 -> 1080 x 1920, T 10).  Per size: device-event times (median, min .. max, every call timed on
its own) of the library with uint8 masks, with bit masks, with `return_tables=True` (no read-back), and of the torch composition; the
peak memory a call allocates above its inputs on both sides; whether the two agree; and the statistics and emit kernels' times (from
torch.profiler's device trace) with the bytes they have to move and the query-pixels they evaluate.

    python tools/vis_time.py [--reps 10] [--out profiles/vis_time.md]
"""
import argparse
import os
import re
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import axial_vs_amd as ax  # noqa: E402
from axial_vs_amd import modules  # noqa: E402
import vis_cases as vc  # noqa: E402

HBM = 8e12
SIZES = [("YTVIS T5: Q100 C40 96x160 -> 384x640 -> 720x1280", vc.Case("ytvis5", 100, 40, 5, 96, 160, (384, 640), (360, 640), (720, 1280), 100, 30, 5, 40, 60)),
         ("YTVIS T5, no empty query: Q100 C40 96x160 -> 384x640 -> 720x1280", vc.Case("ytvis5full", 100, 40, 5, 96, 160, (384, 640), (360, 640), (720, 1280), 100, 30, 5, 40, 0)),
         ("YTVIS T36: Q100 C40 96x160 -> 384x640 -> 720x1280", vc.Case("ytvis36", 100, 40, 36, 96, 160, (384, 640), (360, 640), (720, 1280), 100, 30, 36, 40, 60)),
         ("OVIS-like T10: Q100 C25 90x160 -> 360x640 -> 1080x1920", vc.Case("ovis10", 100, 25, 10, 90, 160, (360, 640), (360, 640), (1080, 1920), 100, 30, 10, 25, 60))]


def mask2bbox(masks):
    """mmdet/core/mask/utils.py:68-89, as it is"""
    N = masks.shape[0]
    bboxes = masks.new_zeros((N, 4), dtype=torch.float32)
    x_any = torch.any(masks, dim=1)
    y_any = torch.any(masks, dim=2)
    for i in range(N):
        x = torch.where(x_any[i, :])[0]
        y = torch.where(y_any[i, :])[0]
        if len(x) > 0 and len(y) > 0:
            bboxes[i, :] = bboxes.new_tensor([x[0], y[0], x[-1] + 1, y[-1] + 1])
    return bboxes


def torch_composition(c, cls, mp):
    """the reference's sequence for one video on the device of its inputs; returns per frame (bbox_results, mask_results)"""
    up = F.interpolate(mp, size=c.bi, mode="bilinear", align_corners=False)[:c.F]
    results = []
    for t in range(c.F):
        m = up[t][:, :c.img[0], :c.img[1]]
        scores = F.softmax(cls, dim=-1)[:, :-1]
        labels = torch.arange(c.C, device=cls.device).unsqueeze(0).repeat(c.Q, 1).flatten(0, 1)
        top, idx = scores.flatten(0, 1).topk(c.K, sorted=False)
        lab = labels[idx]
        m = m[idx // c.C]
        thing = lab < c.things
        top, lab, m = top[thing], lab[thing], m[thing]
        m = F.interpolate(m.unsqueeze(0), size=c.ori, mode="bilinear", align_corners=False).squeeze(0)
        binary = (m > 0).float()
        ms = (m.sigmoid() * binary).flatten(1).sum(1) / (binary.flatten(1).sum(1) + 1e-6)
        binary = binary.bool()
        boxes = torch.cat([mask2bbox(binary), (top * ms)[:, None]], dim=-1)
        boxes = torch.cat([torch.arange(len(boxes), dtype=boxes.dtype, device=boxes.device)[:, None] + 1, boxes], dim=1)
        inds = torch.argsort(boxes[:, -1], descending=True)
        lab, boxes, binary = lab[inds][:c.Ko], boxes[inds][:c.Ko], binary[inds][:c.Ko]
        b, l = boxes.cpu().numpy(), lab.cpu().numpy()
        bbox_results = [b[l == i, :] for i in range(c.things)]
        mask_results = [[] for _ in range(c.things)]
        for j, label in enumerate(lab):
            mask_results[label].append(binary[j].detach().cpu().numpy())
        results.append((bbox_results, mask_results))
    return results


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


def kernel_us(fn):
    """{kernel label: mean device time in us} of the library's kernels over 5 calls, from torch.profiler's device trace; {} without one"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(5):
                fn()
            torch.cuda.synchronize()
        out = {}
        for e in prof.key_averages():
            m = re.search(r"vis_tile_kernel<\s*\d+\s*,\s*(\d)\s*>", e.key)
            label = ("statistics", "emit", "emit")[int(m.group(1))] if m else "candidate" if "vis_candidate" in e.key else "select" if "vis_select" in e.key else None
            if label:
                out[label] = e.device_time_total / max(e.count, 1)
        return out
    except Exception as e:          # no device trace on this installation: the report says so
        print(f"(torch.profiler gave no device trace: {e})", file=sys.stderr)
        return {}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10, help="timed calls of the library path (the torch path gets a third, at least 3)")
    ap.add_argument("--out", default=None, help="also write the report there")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "vis_time.py measures on the GPU"
    old_reps = max(a.reps // 3, 3)
    lines = [f"{torch.cuda.get_device_name(0)}, torch {torch.__version__}; mask logits fp32; max_per_image 100, keep_per_frame 30",
             f"ms per call by device events: median (min .. max) of {a.reps} / {old_reps} calls, each timed on its own", ""]
    table = ["| size | library, uint8 masks | library, bit masks | library, no read-back | torch composition | ratio (uint8 / bits) | peak memory (bits / uint8 / torch) |",
             "|---|---|---|---|---|---|---|"]
    f = lambda t: f"{t[0]:9.3f} ({t[1]:.3f} .. {t[2]:.3f})"
    for name, c in SIZES:
        cls, mp = (x.cuda() for x in vc.make_inputs(c, 7))
        kw = dict(batch_input_shape=c.bi, img_shape=c.img, ori_shape=c.ori, num_things_classes=c.things, num_frames=c.F, max_per_image=c.K, keep_per_frame=c.Ko)
        new8 = lambda: ax.video_instance_inference(cls, mp, **kw)
        newb = lambda: ax.video_instance_inference(cls, mp, mask_format="bits", **kw)
        dev8 = lambda: ax.video_instance_inference(cls, mp, return_tables=True, **kw)
        devb = lambda: ax.video_instance_inference(cls, mp, mask_format="bits", return_tables=True, **kw)
        old = lambda: torch_composition(c, cls, mp)
        t8, tb, td8, tdb, to = timed(new8, a.reps), timed(newb, a.reps), timed(dev8, a.reps), timed(devb, a.reps), timed(old, old_reps, warmup=1)
        mem8, (m8, tab) = peak(dev8)
        memb, _ = peak(devb)
        memo, ref = peak(old)
        # agreement: per frame the non-zero rows in score order -- (label, box) and masks; the inputs are not screened
        tab = {k: v.cpu().numpy() for k, v in tab.items()}
        m8 = m8.cpu().numpy().astype(bool)
        rows_diff = px_diff = 0
        for t, (bbox_results, mask_results) in enumerate(ref):
            rows = np.concatenate([np.concatenate([b, np.full((len(b), 1), i)], axis=1) for i, b in enumerate(bbox_results) if len(b)])
            masks = np.stack([m for per in mask_results for m in per])
            order = np.argsort(-rows[:, 5], kind="stable")
            rows, masks = rows[order], masks[order]
            n = int(min((rows[:, 5] != 0).sum(), (tab["score"][t] > 0).sum()))
            rows_diff += int((rows[:n, 6] != tab["label"][t, :n]).sum() + (rows[:n, 1:5] != tab["bbox"][t, :n]).any(axis=1).sum())
            px_diff += int((masks[:n] != m8[t, :n]).sum())
        us8, usb = kernel_us(dev8), kernel_us(devb)
        nref, P = int(tab["counts"][1]), c.F * c.ori[0] * c.ori[1]
        stat_bytes = c.F * nref * c.h * c.w * 4
        emit_read = c.F * c.Ko * c.h * c.w * 4
        def rate(us, nbytes, evals):
            return (f"{us:8.1f} us; needs {nbytes / 1e6:8.1f} MB: {nbytes / (us * 1e-6) / 1e12:.3f} TB/s = {nbytes / (us * 1e-6) / HBM * 100:.1f}% of 8 TB/s; "
                    f"{evals / 1e6:.0f} M query-pixels: {evals / (us * 1e3):.2f} per ns") if us else "no device trace"
        lines += [f"{name}: masks [{c.F}, {c.Ko}, {c.ori[0]}, {c.ori[1]}], {int(tab['counts'][0])} candidates on {nref} queries",
                  f"    library, uint8 masks read back (one synchronisation) {f(t8)} ms",
                  f"    library, bit masks read back (one synchronisation)   {f(tb)} ms",
                  f"    library, device tensors (return_tables=True): uint8  {f(td8)} ms, bits {f(tdb)} ms",
                  f"    torch composition                                    {f(to)} ms",
                  f"    ratio of the medians: {to[0] / t8[0]:.1f}x with uint8 masks, {to[0] / tb[0]:.1f}x with bit masks (slowest library call against fastest torch call: "
                  f"{to[1] / t8[2]:.1f}x / {to[1] / tb[2]:.1f}x)",
                  f"    peak memory above the inputs: library {memb:.1f} MB (bits) / {mem8:.1f} MB (uint8; the masks themselves: {P * c.Ko / 1e6:.1f} MB), torch composition {memo:.1f} MB",
                  f"    agreement with the torch composition (unscreened inputs): {rows_diff} rows differ in label or box, {px_diff} of {P * c.Ko} mask pixels differ",
                  f"    statistics pass {rate(us8.get('statistics'), stat_bytes, P * nref)}",
                  f"    emit pass, uint8 {rate(us8.get('emit'), emit_read + P * c.Ko, P * c.Ko)}",
                  f"    emit pass, bits  {rate(usb.get('emit'), emit_read + P * c.Ko // 8, P * c.Ko)}",
                  f"    candidate pass {us8.get('candidate', float('nan')):.1f} us, select pass {us8.get('select', float('nan')):.1f} us", ""]
        table.append(f"| {name} | {t8[0]:.2f} ms | {tb[0]:.2f} ms | {td8[0]:.2f} / {tdb[0]:.2f} ms | {to[0]:.1f} ms | {to[0] / t8[0]:.1f}x / {to[0] / tb[0]:.1f}x | "
                     f"{memb:.0f} / {mem8:.0f} / {memo:.0f} MB |")
        del m8, ref
    text = "\n".join(lines + table)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
