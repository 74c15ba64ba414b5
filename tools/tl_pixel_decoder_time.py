"""Time axial_vs_amd.TubeLinkPixelDecoder (eval, HIP) against the same-weights fp32 torch composition (the module's train-mode path,
dropout 0, no grad) and the FPN level alone (axvs_fpn_level_fwd), at the OVIS / YTVIS training crop: T = 4, 384 x 640 (stride-4 map 96 x 160),
6 encoder layers, R50 or Swin-L channel counts.  Prints one JSON line per configuration.

    python tools/tl_pixel_decoder_time.py [--channels r50|swin_l] [--iters 20] [--which all|hip|torch|fpn]
Run each configuration under its own `timeout`."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))     # (tests/golden_util imports the oracle)


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ts = []
    for _ in range(iters):
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        ts.append(ev[0].elapsed_time(ev[1]))
    ts.sort()
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", default="r50", choices=["r50", "swin_l"])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--which", default="all", choices=["all", "hip", "torch", "fpn"])
    a = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    from test_hip_tl_pixel_decoder import make_decoder, feats_for
    ch = (256, 512, 1024, 2048) if a.channels == "r50" else (192, 384, 768, 1536)
    T, H4, W4 = 4, 96, 160
    dec = make_decoder(ch, 6).eval()
    feats = feats_for(ch, T, H4, W4)
    res = {"channels": a.channels, "T": T, "stride4": [H4, W4], "layers": 6}
    if a.which in ("all", "hip"):
        with torch.no_grad():
            res["hip_decoder_ms"] = timed(lambda: dec(feats, T), a.iters)
    if a.which in ("all", "torch"):
        dec.train()
        with torch.no_grad():
            res["torch_fp32_composition_ms"] = timed(lambda: dec(feats, T), max(3, a.iters // 4))
        dec.eval()
    if a.which in ("all", "fpn"):
        import ctypes as C
        from axial_vs_amd import _lib
        L = _lib.lib()
        Cc = 256
        up = torch.randn(T, 48 * 80, Cc, device="cuda")
        pk = dec._pack_fpn(0)
        ws = torch.empty(L.axvs_fpn_level_workspace_bytes(T, H4, W4, ch[0], Cc, 32), dtype=torch.uint8, device="cuda")
        mf = torch.empty(T, Cc, H4, W4, device="cuda")
        st = torch.cuda.current_stream().cuda_stream

        def fpn():
            _lib.check(L.axvs_fpn_level_fwd(feats[0].data_ptr(), up.data_ptr(), 48 * 80 * Cc, Cc, 48, 80, None, mf.data_ptr(), pk.data_ptr(), T, H4, W4,
                                            ch[0], Cc, Cc, 32, 1e-5, 0, ws.data_ptr(), ws.numel(), st), "axvs_fpn_level_fwd")
        res["fpn_level_ms"] = timed(fpn, a.iters)
        flop3 = 2 * T * H4 * W4 * 9 * Cc * Cc
        res["conv3x3_gflop"] = flop3 / 1e9
        import torch.nn.functional as F
        lat, out = dec.lateral_convs[0], dec.output_convs[0]
        upn = up.transpose(1, 2).reshape(T, Cc, 48, 80)
        with torch.no_grad():
            res["torch_fp32_fpn_level_ms"] = timed(lambda: dec.mask_feature(out(lat(feats[0]) + F.interpolate(upn, size=(H4, W4), mode="bilinear",
                                                                                                           align_corners=False))), a.iters)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
