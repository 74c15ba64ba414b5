"""The ConvNeXt / ConvNeXtV2 backbone: `axial_vs_amd.ConvNeXtBackbone` / `ConvNeXtV2Backbone` against the only way to run it without the
library, the reference's op sequence in torch fp32 on the same GPU -- the fp32 restatement of tests/convnext_cases.py (F.pad + F.conv2d
for the patchify layers, a depthwise F.conv2d, F.layer_norm, two F.linear with F.gelu between them, torch.norm for GRN).  The weights
and the input are device tensors before the clock starts.  The restated sequence is the yardstick; the library is never its own
baseline.

Sizes: ConvNeXt-L and ConvNeXtV2-L (depths 3, 3, 27, 3, dims 192 .. 1536) at the VIPSeg clip size -- N 2 frames of 769 x 1345, maps
193 x 337 / 97 x 169 / 49 x 85 / 25 x 43 -- and for one 1281 x 1281 frame.  Reported: device-event times (median, min .. max; every call
timed on its own after warm-up, the same number of calls on both sides, in the same process), kernel launches per call and the
kernel-time shares by kernel name (torch.profiler's device trace), the packed weights' bytes, the workspace's bytes and
torch.cuda.max_memory_allocated over a call, the Linear layers' FLOP count and what the GEMM reaches of the three-piece peak (six bf16
MFMAs per product: 2.5 PFLOP/s / 6), and the fused depthwise kernel's needed traffic (its input rows once, its output rows once)
against HBM.

    python tools/convnext_time.py [--reps 10] [--small] [--out profiles/convnext_time.md]
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
import convnext_cases as cc  # noqa: E402
from axial_vs_amd import _lib, convnext as cx  # noqa: E402

PEAK3 = 2500.0 / 6      # TFLOP/s of fp32 products at six bf16 MFMAs each
HBM = 8000.0            # GB/s


def sizes(small):
    kw = dict(dims=(32, 64, 128, 256), depths=(1, 1, 3, 1)) if small else cc.LARGE
    shapes = [("small", (129, 193), 2)] if small else [("vipseg_clip", (769, 1345), 2), ("frame_1281", (1281, 1281), 1)]
    return [cc.Net(f"{n}_{'v2' if v2 else 'v1'}", 1, s, N, **kw, v2=bool(v2), gamma=True) for n, s, N in shapes for v2 in (0, 1)]


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


def kernels(fn):
    """(launches, {kernel name: total us}) of one call, or None when the profiler gives no device trace"""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            fn()
            torch.cuda.synchronize()
        n, by = 0, {}
        for e in prof.events():
            if str(e.device_type).endswith("CUDA") and e.name and not e.name.startswith(("Memcpy", "Memset")):
                n += 1
                key = e.name.split("(")[0].replace("void ", "").replace("axvs::", "").replace("tr::", "").split("<")[0]
                by[key] = by.get(key, 0.0) + (getattr(e, "device_time", None) or getattr(e, "cuda_time", 0.0))
        return (n, by) if n else None
    except Exception as e:      # noqa: BLE001
        print("profiler unavailable:", e, file=sys.stderr)
        return None


def work(c):
    """(FLOP of the Linear layers, needed bytes of the depthwise kernel, bytes GRN reads again) of one call"""
    flop = dw = grn = 0.0
    maps = cc.map_sizes(*c.size)
    for i, (h, w) in enumerate(maps):
        P, C = c.N * h * w, c.dims[i]
        flop += 2.0 * P * C * (48 if i == 0 else 4 * c.dims[i - 1])
        flop += c.depths[i] * 2 * 2.0 * P * C * 4 * C
        dw += c.depths[i] * 2 * 4.0 * P * C
        grn += c.depths[i] * 4.0 * P * 4 * C if c.v2 else 0.0
    return flop, dw, grn


def measure(c, reps):
    params = cc.net_params(c)
    x = torch.randn(c.N, 3, *c.size, generator=torch.Generator().manual_seed(3)).cuda()
    net = (ax.ConvNeXtV2Backbone(depths=c.depths, dims=c.dims) if c.v2 else ax.ConvNeXtBackbone(depths=c.depths, dims=c.dims))
    net.load_state_dict(params)
    net = net.cuda().eval()
    r32 = cc.Restatement({k: v.cuda() for k, v in params.items()}, torch.float32)
    del params
    names = ("res2", "res3", "res4", "res5")
    lib = lambda: net(x)
    ref = lambda: r32.forward(x, c.depths)
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
    maps = cc.map_sizes(*c.size)
    cfg = cx._cfg(c.N, *c.size, maps, c.depths, c.dims, c.v2)
    packed, ws = _lib.lib().axvs_cnx_packed_bytes(ctypes.byref(cfg)), _lib.lib().axvs_cnx_workspace_bytes(ctypes.byref(cfg))
    flop, dwb, grnb = work(c)
    lines = [f"## {c.name}: {'ConvNeXtV2' if c.v2 else 'ConvNeXt'}, depths {list(c.depths)}, dims {list(c.dims)}, N {c.N} frames of {c.size[0]} x {c.size[1]}, maps {maps}", "",
             "| | time per call | kernel launches | max_memory_allocated over a call |", "|---|---|---|---|",
             f"| library | {t_lib[0]:.3f} ({t_lib[1]:.3f} .. {t_lib[2]:.3f}) | {k_lib[0] if k_lib else 'n/a'} | {m_lib / 2**20:.1f} MiB (workspace included) |",
             f"| torch sequence (fp32 restatement) | {t_ref[0]:.3f} ({t_ref[1]:.3f} .. {t_ref[2]:.3f}) | {k_ref[0] if k_ref else 'n/a'} | {m_ref / 2**20:.1f} MiB |", "",
             f"library / torch = {t_lib[0] / t_ref[0]:.2f}.  Packed weights {packed / 1e6:.1f} MB beside the parameters, workspace {ws / 1e6:.1f} MB.  "
             f"Linear layers: {flop / 1e12:.3f} TFLOP per call.  max |library - torch| per output (both fp32, each with its own rounding): "
             f"{', '.join(f'{k} {v:.2e} (of {mags[k]:.1f})' for k, v in errs.items())}.", ""]
    if k_lib:
        tot = sum(k_lib[1].values())
        lines += ["library kernel time by kernel (one call, device trace):", "", "| kernel | us | share |", "|---|---|---|"]
        lines += [f"| {k} | {v:.0f} | {100 * v / tot:.0f} % |" for k, v in sorted(k_lib[1].items(), key=lambda kv: -kv[1])]
        lines += ["", f"sum of kernel times {tot / 1e3:.3f} ms against {t_lib[0]:.3f} ms wall over {k_lib[0]} launches.", ""]
        g, d = k_lib[1].get("tr_gemm_nt_kernel", 0.0), k_lib[1].get("cnx_dwln_kernel", 0.0)
        if g:
            lines += [f"GEMM: {flop / 1e12:.3f} TFLOP in {g / 1e3:.3f} ms = {flop / g / 1e6:.1f} TFLOP/s of fp32 products, {100 * flop / g / 1e6 / PEAK3:.0f} % of the "
                      f"three-piece peak ({PEAK3:.0f} TFLOP/s: 2.5 PFLOP/s of bf16 MFMA, six per product)."]
        if d:
            lines += [f"Depthwise 7x7 + LayerNorm ({sum(c.depths)} launches): {dwb / 1e6:.0f} MB needed (input rows once, output rows once) in {d / 1e3:.3f} ms = "
                      f"{dwb / d / 1e3:.0f} GB/s, {100 * dwb / d / 1e3 / HBM:.0f} % of {HBM / 1e3:.0f} TB/s HBM."]
        if c.v2:
            s = sum(k_lib[1].get(k, 0.0) for k in ("cnx_sumsq_kernel", "cnx_grn_scale_kernel", "cnx_scale_w_kernel"))
            lines += [f"GRN (a pass of its own over the hidden rows, {grnb / 1e6:.0f} MB read again; the scale goes into a per-frame copy of W2): "
                      f"{s / 1e3:.3f} ms in all, {100 * s / tot:.1f} % of the kernel time."]
        lines += [""]
    if k_ref:
        tot = sum(k_ref[1].values())
        top = sorted(k_ref[1].items(), key=lambda kv: -kv[1])[:6]
        lines += [f"torch sequence ({k_ref[0]} launches), the six largest kernels: " + "; ".join(f"{k[:60]} {100 * v / tot:.0f} %" for k, v in top) + f" of {tot / 1e3:.3f} ms.", ""]
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "convnext_time.md"))
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    lines = ["# ConvNeXt backbone: library vs the reference's op sequence in torch (fp32), same GPU, same process", "",
             f"`python tools/convnext_time.py --reps {a.reps}{' --small' if a.small else ''}` on {torch.cuda.get_device_name(0)}; times in ms: median "
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
