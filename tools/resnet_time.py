"""The ResNet bottleneck backbone: `axial_vs_amd.ResNetBackbone` (R-50) against the only way to run it without the library, the reference's
op sequence in torch fp32 on the same GPU -- the fp32 restatement of tests/resnet_cases.py (F.conv2d, eval F.batch_norm, ReLU,
F.max_pool2d, the sum with the shortcut).  The weights and the input are device tensors before the clock starts.  The restated sequence
is the yardstick; the library is never its own baseline.

Sizes: R-50 at the VIPSeg clip size -- N 2 frames of 769 x 1345, maps 193 x 337 / 97 x 169 / 49 x 85 / 25 x 43 -- and for one 1281 x 1281
frame.  Reported: device-event times (median, min .. max; every call timed on its own after warm-up, the same number of calls on both
sides, in the same process), kernel launches per call and the kernel-time shares by kernel name (torch.profiler's device trace), the
packed weights' bytes, the workspace's bytes and torch.cuda.max_memory_allocated over a call; for the 3x3 kernel per stage, from the
per-launch device trace of whole calls: its time, what it reaches of the three-piece peak (six bf16 MFMAs per product: 2.5 PFLOP/s / 6),
its MFMA and traffic floors, its grid's fill and the distance to the nearest floor; for the stem its time against its floors.

    python tools/resnet_time.py [--reps 10] [--small] [--out profiles/resnet_time.md]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o rn -- python <a script that calls the module>     # a run of its own
    python tools/resnet_time.py --stats-csv DIR/rn_kernel_stats.csv --out profiles/resnet_time.md                      # appends its table
    python tools/resnet_time.py --resources-text FILE --out profiles/resnet_time.md                                    # appends the register remarks
"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import axial_vs_amd as ax  # noqa: E402
import resnet_cases as rc  # noqa: E402
from axial_vs_amd import _lib  # noqa: E402

# the MI355X datasheet's figures: 2.5 PFLOP/s of dense bf16 MFMA, 8 TB/s of HBM3E
PEAK3 = 2500.0 / 6      # TFLOP/s of fp32 products at six bf16 MFMAs each
HBM = 8000.0            # GB/s
R50 = dict(stem=64, widths=(64, 128, 256, 512), outs=(256, 512, 1024, 2048), blocks=(3, 4, 6, 3))
SMALL = dict(stem=32, widths=(32, 64, 128, 256), outs=(128, 256, 512, 1024), blocks=(1, 1, 2, 1))


def sizes(small):
    kw = SMALL if small else R50
    shapes = [("small", (129, 193), 2)] if small else [("vipseg_clip", (769, 1345), 2), ("frame_1281", (1281, 1281), 1)]
    return [rc.Net(n, 1, s, N, **kw, stride_in_1x1=False, res5_dilation=1) for n, s, N in shapes]


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts), max(ts)


def peak_above(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def kernels(fn, calls=5):
    """(launches of one call, {kernel name: total us of one call}, [(kernel name, median us over `calls` calls) in launch order]), or None when the
    profiler gives no device trace"""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        runs = []
        for _ in range(calls):
            with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
                fn()
                torch.cuda.synchronize()
            ev = [e for e in prof.events() if str(e.device_type).endswith("CUDA") and e.name and not e.name.startswith(("Memcpy", "Memset"))]
            ev.sort(key=lambda e: e.time_range.start)
            runs.append([(e.name.split("(")[0].replace("void ", "").replace("axvs::", "").replace("tr::", "").split("<")[0],
                          getattr(e, "device_time", None) or getattr(e, "cuda_time", 0.0)) for e in ev])
        if not runs[0]:
            return None
        runs = [r for r in runs if [k for k, _ in r] == [k for k, _ in runs[0]]]      # (calls whose launch sequence is the first call's)
        order = [(runs[0][i][0], statistics.median(r[i][1] for r in runs)) for i in range(len(runs[0]))]
        by = {}
        for k, v in order:
            by[k] = by.get(k, 0.0) + v
        return len(order), by, order
    except Exception as e:      # noqa: BLE001
        print("profiler unavailable:", e, file=sys.stderr)
        return None


# workgroups of rn_conv3_kernel<stride, channel tile> a compute unit holds: what its registers allow (the register table at the end of
# profiles/resnet_time.md; LDS, at most 74 KiB per workgroup, allows as many)
CONV3_PER_CU = {(1, 64): 2, (1, 128): 1, (2, 64): 2, (2, 128): 2}
CUS = 256


def conv3_blocks(c):
    """every block's 3x3 in launch order: (stage, block, input map, stride, C, channel tile, workgroups, FLOP, needed bytes)"""
    out = []
    maps = rc.stage_sizes(c, *c.size)
    strides = rc.strides_of(c)
    for i in range(4):
        C = c.widths[i]
        for j in range(c.blocks[i]):
            s = strides[i] if j == 0 else 1
            h, w = maps[i] if j == 0 else maps[i + 1]
            ho, wo = -(-h // s), -(-w // s)
            wgs = lambda bn: c.N * -(-C // bn) * -(-ho // (8 if s == 1 else 4)) * -(-wo // 16)
            bn = 128 if C > 64 and wgs(128) >= 256 else 64
            out.append((i, j, (h, w), s, C, bn, wgs(bn), 2.0 * c.N * ho * wo * C * C * 9, 4.0 * c.N * (h * w + ho * wo) * C + 6.0 * 9 * C * C))
    return out


def conv3_section(c, order):
    """the per-stage table of the 3x3 kernel from the per-launch device trace of whole calls"""
    times = [v for k, v in order if k == "rn_conv3_kernel"]
    blocks = conv3_blocks(c)
    if len(times) != len(blocks):
        return [f"3x3 kernel: the trace holds {len(times)} launches for {len(blocks)} blocks; no per-stage table.", ""]
    lines = ["3x3 kernel per stage, from the device trace of whole calls (each launch's median over five calls, in launch order; a stage's later blocks: their",
             "mean).  MFMA floor = the products at the three-piece peak; traffic floor = input rows once + output rows once + split weights once at 8 TB/s; grid",
             f"fill = workgroups over the slots of the rounds they take on {CUS} compute units that hold 1 or 2 workgroups of the form (by its registers).", "",
             "| blocks | launches | map | form <stride, channels> | workgroups (per CU) | grid fill | us per launch | TFLOP/s of fp32 products | of the three-piece peak | "
             "MFMA floor us | traffic floor us | nearest floor, and the distance to it |", "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    groups = {}
    for b, t in zip(blocks, times):
        groups.setdefault((b[0], b[1] > 0), []).append((b, t))
    total = 0.0
    for (i, later), items in groups.items():
        b = items[0][0]
        t = sum(x[1] for x in items) / len(items)
        total += sum(x[1] for x in items)
        _, _, (h, w), s, C, bn, wg, flop, need = b
        per = CONV3_PER_CU[(s, bn)]
        fill = wg / (-(-wg // (CUS * per)) * CUS * per)
        f_mfma, f_mem = flop / PEAK3 / 1e6, need / HBM / 1e3
        name = f"res{i + 2}.0" if not later else f"res{i + 2}.1 .. {c.blocks[i] - 1}"
        lines.append(f"| {name} | {len(items)} | {h} x {w} x {C}, stride {s} | <{s}, {bn}> | {wg} ({per}) | {100 * fill:.0f} % | {t:.1f} | {flop / t / 1e6:.1f} | "
                     f"{100 * flop / t / 1e6 / PEAK3:.0f} % | {f_mfma:.1f} | {f_mem:.1f} | {'MFMA issue' if f_mfma >= f_mem else 'traffic'}, {t / max(f_mfma, f_mem):.1f} x |")
    lines += ["", f"all {len(times)} 3x3 launches of a call: {total / 1e3:.3f} ms.  The table states which floor is nearest and how far each stage is from it, and how much of that the "
              "grid's fill accounts for (a stage at 50 % fill cannot come nearer than 2 x).  The rest of the distance -- waiting at the two barriers of a chunk around the "
              "staging phase, and for the weight fragments of the next (chunk, tap) step -- is not split further: no counter run was made, so it is unmeasured.", ""]
    return lines


def measure(c, reps):
    params = rc.net_params(c)
    x = torch.randn(c.N, 3, *c.size, generator=torch.Generator().manual_seed(3)).cuda()
    net = ax.ResNetBackbone(depth=None, num_blocks=c.blocks, stem_out_channels=c.stem, bottleneck_channels=c.widths, stage_out_channels=c.outs)
    net.load_state_dict(params)
    net = net.cuda().eval()
    r32 = rc.restatement(c, {k: v.cuda() for k, v in params.items()}, torch.float32)
    del params
    names = ("res2", "res3", "res4", "res5")
    lib = lambda: net(x)
    ref = lambda: r32.forward(x, c.blocks)
    got, want = lib(), ref()
    errs = {k: float((got[k] - want[k]).abs().max()) for k in names}
    mags = {k: float(want[k].abs().max()) for k in names}
    del got, want
    t_lib, t_ref = timed(lib, reps), timed(ref, reps)
    from axial_vs_amd import modules
    modules._workspaces.clear()
    torch.cuda.empty_cache()
    m_lib, m_ref = peak_above(lib), peak_above(ref)
    k_lib, k_ref = kernels(lib), kernels(ref)
    maps = rc.stage_sizes(c, *c.size)
    cfg = net._conf.cfg(c.N, *c.size, maps[:4])
    packed, ws = _lib.lib().axvs_rn_packed_bytes(ctypes.byref(cfg)), _lib.lib().axvs_rn_workspace_bytes(ctypes.byref(cfg))
    lines = [f"## {c.name}: blocks {list(c.blocks)}, bottleneck widths {list(c.widths)}, N {c.N} frames of {c.size[0]} x {c.size[1]}, maps {maps[1:]}", "",
             "| | time per call | kernel launches | max_memory_allocated over a call |", "|---|---|---|---|",
             f"| library | {t_lib[0]:.3f} ({t_lib[1]:.3f} .. {t_lib[2]:.3f}) | {k_lib[0] if k_lib else 'n/a'} | {m_lib / 2**20:.1f} MiB (workspace included) |",
             f"| torch sequence (fp32 restatement) | {t_ref[0]:.3f} ({t_ref[1]:.3f} .. {t_ref[2]:.3f}) | {k_ref[0] if k_ref else 'n/a'} | {m_ref / 2**20:.1f} MiB |", "",
             f"library / torch = {t_lib[0] / t_ref[0]:.2f}.  Packed weights {packed / 1e6:.1f} MB beside the parameters, workspace {ws / 1e6:.1f} MB.  "
             f"max |library - torch| per output (both fp32, each with its own rounding): "
             f"{', '.join(f'{k} {v:.2e} (of {mags[k]:.1f})' for k, v in errs.items())}.", ""]
    if k_lib:
        tot = sum(k_lib[1].values())
        lines += ["library kernel time by kernel (one call, device trace):", "", "| kernel | us | share |", "|---|---|---|"]
        lines += [f"| {k} | {v:.0f} | {100 * v / tot:.0f} % |" for k, v in sorted(k_lib[1].items(), key=lambda kv: -kv[1])]
        lines += ["", f"sum of kernel times {tot / 1e3:.3f} ms against {t_lib[0]:.3f} ms wall over {k_lib[0]} launches.", ""]
        st = k_lib[1].get("rn_stem_kernel", 0.0)
        if st:
            hp, wp = maps[0]
            px = c.N * ((c.size[0] + 1) // 2) * ((c.size[1] + 1) // 2)
            outb, inb, mid = 4.0 * c.N * hp * wp * c.stem, 4.0 * c.N * 3 * c.size[0] * c.size[1], 4.0 * px * c.stem
            flop = 2.0 * 147 * c.stem * px
            t_traffic, t_mfma = (inb + outb) / HBM / 1e3, 2.0 * 160 * c.stem * px / PEAK3 / 1e6      # us
            near = ("MFMA issue", t_mfma) if t_mfma >= t_traffic else ("traffic", t_traffic)
            lines += [f"Stem (one launch, three-piece MFMA, K = 147 padded to 160): {st:.0f} us = {100 * st / tot:.1f} % of the call's kernel time, for {flop / 1e9:.1f} GFLOP "
                      f"= {flop / st / 1e6:.1f} TFLOP/s of fp32 products.  MFMA floor {t_mfma:.0f} us ({100 * t_mfma / st:.0f} % of the three-piece peak reached); it reads "
                      f"{inb / 1e6:.0f} MB and writes {outb / 1e6:.0f} MB: {t_traffic:.1f} us at {HBM / 1e3:.0f} TB/s.  Nearest floor: {near[0]}, {st / near[1]:.1f} x away; the "
                      f"rest (the per-lane gather of the patch values from LDS and their split, once per step and m-tile) is not split further.  The stride-2 map the "
                      f"kernel keeps in LDS would be {mid / 1e6:.0f} MB written and read again by a separate pool kernel ({2 * mid / HBM / 1e3:.0f} us at "
                      f"{HBM / 1e3:.0f} TB/s).", ""]
        lines += conv3_section(c, k_lib[2])
    if k_ref:
        tot = sum(k_ref[1].values())
        top = sorted(k_ref[1].items(), key=lambda kv: -kv[1])[:6]
        lines += [f"torch sequence ({k_ref[0]} launches), the six largest kernels: " + "; ".join(f"{k[:60]} {100 * v / tot:.0f} %" for k, v in top) + f" of {tot / 1e3:.3f} ms.", ""]
    return lines


def stats_table(path):
    """the per-kernel table of one separate `rocprofv3 --kernel-trace --stats` run (its kernel_stats csv), as markdown"""
    import csv
    with open(path) as f:
        rows = list(csv.DictReader(f))
    lines = ["## one separate `rocprofv3 --kernel-trace --stats` run: four library calls at the VIPSeg clip size, the pack included", "",
             "| kernel | calls | total ms | average us | share |", "|---|---|---|---|---|"]
    for r in rows[:12]:
        name = r["Name"].split("(")[0].replace("void ", "").replace("axvs::", "").replace("tr::", "")[:70]
        lines.append(f"| {name} | {r['Calls']} | {float(r['TotalDurationNs']) / 1e6:.3f} | {float(r['AverageNs']) / 1e3:.1f} | {float(r['Percentage']):.1f} % |")
    return lines + [""]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resnet_time.md"))
    ap.add_argument("--stats-csv", help="append the table of a rocprofv3 kernel_stats csv to --out and stop")
    ap.add_argument("--resources-text", help="append a text file (the compiler's register remarks of the unit) to --out and stop")
    a = ap.parse_args()
    if a.stats_csv or a.resources_text:
        with open(a.out, "a") as f:
            if a.stats_csv:
                f.write("\n".join(stats_table(a.stats_csv)) + "\n")
            if a.resources_text:
                f.write(open(a.resources_text).read())
        return
    torch.set_grad_enabled(False)
    lines = ["# ResNet-50 backbone: library vs the reference's op sequence in torch (fp32), same GPU, same process", "",
             f"`python tools/resnet_time.py --reps {a.reps}{' --small' if a.small else ''}` on {torch.cuda.get_device_name(0)}; times in ms: median "
             "(min .. max).", ""]
    for c in sizes(a.small):
        lines += measure(c, a.reps)
        print(f"{c.name}: measured", file=sys.stderr, flush=True)
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
