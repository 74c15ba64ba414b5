"""Tube-Link's per-clip query decoder: `axial_vs_amd.TubeLinkClipDecoder` against the only way to run it without the library, the
reference's op sequence in torch on the same GPU -- the fp32 restatement of tests/m2f_decoder_cases.py (level embedding, 3-D sine
embedding, and per layer the full-resolution mask einsum, F.interpolate, threshold, the 8-head mask copy, nn.MultiheadAttention's
forward, LayerNorms, FFN).  Everything the reference does per forward is inside the timed call and runs on the GPU, as it does there:
the level embedding, the 3-D sine embedding from torch ops on the device, the token transposes.  The weights and inputs are device
tensors before the clock starts.  The restated sequence is the yardstick; the library is never its own baseline.  Two things the
restatement leaves out make it slightly cheaper than the reference itself: the class logits of every mask head, and the sigmoid before
the threshold.

Sizes: the YouTube-VIS 2021 size (Q 100, 3 frames per clip, mask features 96 x 160 x 256, levels 12 x 20 / 24 x 40 / 48 x 80, 9 layers)
for 1 clip and 3 stacked clips (the torch side loops over the clips, as the reference does), and an OVIS-like pyramid (mask features
192 x 320, levels 24 x 40 / 48 x 80 / 96 x 160).  Per size: device-event times (median, min .. max; every call timed on its own after
warm-up, the same number of calls on both sides, in the same process), kernel launches per call and the kernel-time shares by kernel name (torch.profiler's device
trace), the peak memory a call allocates above its inputs, and how the two sides agree: the difference of the queries, the number of
attention-mask bits in which the library's free run differs from the torch side's (a flipped bit, not rounding, is what moves a query by
more than ~1e-5), and whether the stacked call equals the single-clip calls bit for bit.

    python tools/m2f_decoder_time.py [--reps 20] [--out profiles/m2f_decoder_time.md]
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
import m2f_decoder_cases as mc  # noqa: E402

SIZES = [("YTVIS21, 1 clip", mc.Case("ytvis1", 1, 1, 100, 3, (96, 160), ((12, 20), (24, 40), (48, 80)), 9, 40, 0.0)),
         ("YTVIS21, 3 clips stacked", mc.Case("ytvis3", 1, 3, 100, 3, (96, 160), ((12, 20), (24, 40), (48, 80)), 9, 40, 0.0)),
         ("OVIS-like, 1 clip", mc.Case("ovis1", 1, 1, 100, 3, (192, 320), ((24, 40), (48, 80), (96, 160)), 9, 25, 0.0))]
ORDER = ("cross_attn", "norm", "self_attn", "norm", "ffn", "norm")


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
                key = e.name.split("<")[0].split("(")[0].replace("void ", "").replace("axvs::", "").replace("tr::", "")
                by[key] = by.get(key, 0.0) + (getattr(e, "device_time", None) or getattr(e, "cuda_time", 0.0))
        return (n, by) if n else None
    except Exception as e:      # noqa: BLE001
        print("profiler unavailable:", e, file=sys.stderr)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "m2f_decoder_time.md"))
    ap.add_argument("--sizes", default="0,1,2")
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    lines = ["# Per-clip query decoder: library vs the reference's op sequence in torch (fp32), same GPU, same process", "",
             f"`python tools/m2f_decoder_time.py --reps {a.reps}` on {torch.cuda.get_device_name(0)}; times in ms: median (min .. max).", ""]
    for idx in [int(s) for s in a.sizes.split(",")]:
        title, c = SIZES[idx]
        params = {k: v.cuda() for k, v in mc.make_params(c).items()}
        mf, mems = mc.make_inputs(c)
        mf, mems = mf.cuda(), [m.cuda() for m in mems]
        dec = ax.TubeLinkClipDecoder(c.Q, c.K, transformer_decoder=dict(num_layers=c.layers, transformerlayers=dict(
            attn_cfgs=dict(embed_dims=256, num_heads=8), ffn_cfgs=dict(embed_dims=256, feedforward_channels=2048), operation_order=ORDER)))
        dec.load_state_dict({k: v.cpu() for k, v in params.items()})
        dec = dec.cuda()

        def lib():
            return dec(mf, mems)

        def lib_pred():
            return dec(mf, mems, return_predictions=True)

        def torch_run():      # the reference loops over the clips
            return [mc.Restatement(params, mf[n:n + 1], [m[n:n + 1] for m in mems], torch.float32, c.layers).run() for n in range(c.N)]

        def torch_seq():
            return torch.cat([r[1] for r in torch_run()], dim=1)

        try:
            ref = torch_seq()
        except torch.cuda.OutOfMemoryError:
            lines += [f"## {title}", "", "the torch sequence does not fit", ""]
            continue
        got = lib()
        err = float((got - ref).abs().max())
        # attention-mask bits: the library's free run against the torch side's, layer by layer
        from axial_vs_amd.clip_decoder import unpack_mask_bits
        recs = torch_run()
        _, lm = dec(mf, mems, return_masks=True)
        nbits = ndiff = 0
        for i, (bits, _) in enumerate(lm):
            want = torch.cat([r[0][i]["logits"] < 0 for r in recs], dim=0)
            have = unpack_mask_bits(bits, mc.keys_of(c, i % 3))
            nbits += want.numel()
            ndiff += int((have != want).sum())
        del recs, lm
        stacked = all(torch.equal(dec(mf[n:n + 1], [m[n:n + 1] for m in mems])[:, 0], got[:, n]) for n in range(c.N)) if c.N > 1 else None
        t_lib, t_pred, t_ref = timed(lib, a.reps), timed(lib_pred, a.reps), timed(torch_seq, a.reps)
        m_lib, m_ref = peak_above(lib), peak_above(torch_seq)
        k_lib, k_ref = kernels(lib), kernels(torch_seq)
        keys = [mc.keys_of(c, l) for l in range(3)]
        lines += [f"## {title}: N {c.N}, Q {c.Q}, T {c.T}, mask features {c.hw[0]} x {c.hw[1]}, keys per level {keys}, {c.layers} layers", "",
                  "| | time | kernel launches | peak memory above the inputs |", "|---|---|---|---|",
                  f"| library, query_feat only | {t_lib[0]:.3f} ({t_lib[1]:.3f} .. {t_lib[2]:.3f}) | {k_lib[0] if k_lib else 'n/a'} | {m_lib / 2**20:.1f} MiB |",
                  f"| library, with the last layer's predictions | {t_pred[0]:.3f} ({t_pred[1]:.3f} .. {t_pred[2]:.3f}) | | |",
                  f"| torch sequence | {t_ref[0]:.3f} ({t_ref[1]:.3f} .. {t_ref[2]:.3f}) | {k_ref[0] if k_ref else 'n/a'} | {m_ref / 2**20:.1f} MiB |", "",
                  f"library / torch = {t_lib[0] / t_ref[0]:.2f}; max |library - torch| on query_feat = {err:.2e}; {ndiff} of {nbits} attention-mask bits "
                  "differ between the two free runs (fp32 against fp32: both carry their own rounding, and a logit inside the band may fall on either side)"
                  + ("" if stacked is None else f"; the stacked call equals the {c.N} single-clip calls bit for bit: {stacked}"), ""]
        if k_lib:
            tot = sum(k_lib[1].values())
            lines += ["library kernel time by kernel (one call, device trace):", "", "| kernel | us | share |", "|---|---|---|"]
            lines += [f"| {k} | {v:.0f} | {100 * v / tot:.0f} % |" for k, v in sorted(k_lib[1].items(), key=lambda kv: -kv[1])]
            lines += ["", f"sum of kernel times {tot / 1e3:.3f} ms against {t_lib[0]:.3f} ms wall over {k_lib[0]} dependent launches "
                      "(equal: the kernels run back to back and the time is inside them; less: the rest is gaps between launches)", ""]
        del dec, params, mf, mems
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
