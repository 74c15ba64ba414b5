"""Video-kMaX's pixel decoder: `axial_vs_amd.KMaXPixelDecoder` against the only way to run it without the library, the reference's op
sequence in torch on the same GPU -- the fp32 restatement of tests/kmax_pixel_decoder_cases.py (per axis pass the [N, 24, L, L]
similarity tensor and three gathered [L, L, d] position tables; fp32 convolutions followed by separate BatchNorm and GELU kernels).  The
weights and inputs are device tensors before the clock starts.  The restated sequence is the yardstick; the library is never its own
baseline.

Sizes: VIPSeg R50 -- T 2, 769 x 1345, maps 25 x 43 / 49 x 85 / 97 x 169 / 193 x 337, in_channels (2048, 1024, 512, 256), the shipped
configuration; and one 1281 x 1281 frame (maps 41 / 81 / 161 / 321 squared).  Reported: device-event times (median, min .. max; every
call timed on its own after warm-up, the same number of calls on both sides, in the same process), kernel launches per call and the
kernel-time shares by kernel name (torch.profiler's device trace), torch.cuda.max_memory_allocated over a call above what was allocated
before it (the library's workspace is allocated inside the measured call: the cache is dropped first), how the two sides agree, and what
the attention kernel reaches.

    python tools/kmax_pixel_decoder_time.py [--reps 20] [--out profiles/kmax_pixel_decoder_time.md]
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
import kmax_pixel_decoder_cases as pc  # noqa: E402

SHIPPED = dict(in_channels=(256, 512, 1024, 2048), dec_layers=(1, 5, 1, 1), dec_channels=(512, 256, 128, 64),
               layer_types=("axial", "axial", "bottleneck", "bottleneck"))
SIZES = [pc.Case("vipseg_r50", 1, (769, 1345), 2, **SHIPPED), pc.Case("frame_1281", 1, (1281, 1281), 1, **SHIPPED)]
SMALL = [pc.Case("small", 1, (129, 193), 2, **SHIPPED)]      # --small: a dry run


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
                key = e.name.split("(")[0].replace("void ", "").replace("axvs::", "").replace("tr::", "")
                key = key if key.startswith("kpix_axial_attn") else key.split("<")[0]
                by[key] = by.get(key, 0.0) + (getattr(e, "device_time", None) or getattr(e, "cuda_time", 0.0))
        return (n, by) if n else None
    except Exception as e:      # noqa: BLE001
        print("profiler unavailable:", e, file=sys.stderr)
        return None


def attention_work(c):
    """(MFMA flop, bytes of qkv rows read and output rows written) of the twelve axis passes"""
    flop = byts = 0.0
    for i, (h, w) in enumerate(pc.query_shapes(c.spatial)):
        if c.layer_types[i] != "axial":
            continue
        b = c.dec_channels[i]
        dk, dv = b // 8, b // 4
        for L, nseq in ((h, c.N * w), (w, c.N * h)):
            L16 = (L + 15) // 16 * 16
            per_head = 2.0 * L16 * L16 * dk * 5 + 2.0 * L16 * L16 * dv + 2.0 * L16 * (L16 + 16) * dv      # content + 2 x 2 position tiles; W v; skewed W x window
            flop += c.dec_layers[i] * nseq * 8 * per_head
            byts += c.dec_layers[i] * nseq * L * 4.0 * (4 * b + 2 * b)
    return flop, byts


def measure(c, reps):
    params = pc.make_params(c)
    feats = {k: v.cuda() for k, v in pc.make_inputs(c).items()}
    dec = ax.KMaXPixelDecoder(pc.input_shape(c), c.dec_layers, c.dec_channels, c.layer_types, c.spatial)
    dec.load_state_dict(params)
    dec = dec.cuda().eval()
    r32 = pc.Restatement({k: v.cuda() for k, v in params.items()}, torch.float32)
    lib = lambda: dec.forward_features(dict(feats))
    ref = lambda: r32.run(feats, c.dec_layers)[1]
    pan, _, ms = lib()
    want = ref()
    errs = {k: float((g - w).abs().max()) for k, g, w in zip(pc.OUTPUTS, list(ms) + [pan], want)}
    mags = {k: float(w.abs().max()) for k, w in zip(pc.OUTPUTS, want)}
    del want, pan, ms
    t_lib, t_ref = timed(lib, reps), timed(ref, reps)
    from axial_vs_amd import modules
    modules._workspaces.clear()
    torch.cuda.empty_cache()
    m_lib, m_ref = peak_above(lib), peak_above(ref)
    k_lib, k_ref = kernels(lib), kernels(ref)
    sizes = pc.query_shapes(c.spatial)
    lines = [f"## {c.name}: N {c.N} frames of {c.spatial[0]} x {c.spatial[1]}, maps {sizes}, in_channels {list(c.in_channels[::-1])}, dec_layers "
             f"{list(c.dec_layers)}, dec_channels {list(c.dec_channels)}", "",
             "| | time per call | kernel launches | max_memory_allocated over a call |", "|---|---|---|---|",
             f"| library | {t_lib[0]:.3f} ({t_lib[1]:.3f} .. {t_lib[2]:.3f}) | {k_lib[0] if k_lib else 'n/a'} | {m_lib / 2**20:.1f} MiB (workspace included) |",
             f"| torch sequence (fp32 restatement) | {t_ref[0]:.3f} ({t_ref[1]:.3f} .. {t_ref[2]:.3f}) | {k_ref[0] if k_ref else 'n/a'} | {m_ref / 2**20:.1f} MiB |", "",
             f"library / torch = {t_lib[0] / t_ref[0]:.2f}.  max |library - torch| per output (both fp32, each with its own rounding): "
             f"{', '.join(f'{k} {v:.2e} (of {mags[k]:.1f})' for k, v in errs.items())}.", ""]
    if k_lib:
        tot = sum(k_lib[1].values())
        lines += ["library kernel time by kernel (one call, device trace):", "", "| kernel | us | share |", "|---|---|---|"]
        lines += [f"| {k} | {v:.0f} | {100 * v / tot:.0f} % |" for k, v in sorted(k_lib[1].items(), key=lambda kv: -kv[1])]
        lines += ["", f"sum of kernel times {tot / 1e3:.3f} ms against {t_lib[0]:.3f} ms wall over {k_lib[0]} launches.", ""]
        att = sum(v for k, v in k_lib[1].items() if k.startswith("kpix_axial_attn"))
        if att:
            flop, byts = attention_work(c)
            lines += [f"attention kernel ({2 * sum(n for n, t in zip(c.dec_layers, c.layer_types) if t == 'axial')} launches): {att:.0f} us for {flop / 1e9:.2f} GFLOP of "
                      f"f32-input MFMA (pad rows and the unused half of the position tiles included) and {byts / 2**20:.1f} MiB of rows: {flop / att / 1e6:.1f} TFLOP/s "
                      f"({100 * flop / att / 1e6 / 157.3:.0f} % of the 157.3 TFLOP/s f32-input MFMA peak), {byts / att / 1e3:.1f} GB/s "
                      f"({100 * byts / att / 1e3 / 8000:.0f} % of 8 TB/s HBM).", ""]
    if k_ref:
        tot = sum(k_ref[1].values())
        top = sorted(k_ref[1].items(), key=lambda kv: -kv[1])[:6]
        lines += ["torch sequence, the six largest kernels: " + "; ".join(f"{k[:60]} {100 * v / tot:.0f} %" for k, v in top) + f" of {tot / 1e3:.3f} ms.", ""]
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmax_pixel_decoder_time.md"))
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    lines = ["# pixel decoder: library vs the reference's op sequence in torch (fp32), same GPU, same process", "",
             f"`python tools/kmax_pixel_decoder_time.py --reps {a.reps}{' --small' if a.small else ''}` on {torch.cuda.get_device_name(0)}; times in ms: median "
             "(min .. max).", ""]
    for c in (SMALL if a.small else SIZES):
        lines += measure(c, a.reps)
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
