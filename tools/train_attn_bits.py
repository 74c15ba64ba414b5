"""Bit record of the training tier's spatial-attention kernels: forward + backward of a fixed list of cases (fixed data and
dropout seeds) that between them reach every spatial kernel of axvs_train.h and the edges inside it, one SHA-256 per tensor --
the outputs, d_src, d_pos (d_clip_query) and every parameter gradient.  Two libraries compute the same bits iff their outputs are the
same text:

    AXVS_LIB_PATH=tools/ab/parent.so python3 tools/train_attn_bits.py > a.txt;  python3 tools/train_attn_bits.py > b.txt;  cmp a.txt b.txt

kind, (B, T, C, H, W), heads, d_ffn, p_dropout, p_attn_drop, train_valu -- and what the case reaches:"""
import hashlib, json, os, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "oracle"))
import axvs_oracle as orc
import axial_vs_amd as ax
from axial_vs_amd import _lib

CASES = [
    # split forward + LDS-resident backward; frames of 5 keys: one masked key tile
    ("axial", (2, 2, 256, 16, 5), 8, 256, 0.3, 0.1, 0),
    # 75 and 129 queries, ragged frames; S * heads = 344 and 200 < 512: the grid is split over query tiles and frames
    ("axial", (1, 3, 256, 25, 43), 8, 256, 0.1, 0.1, 0),
    # 240 keys: the LDS-resident fp32 forward and backward; N = 960 > 512: the key side stages its queries in two chunks
    ("full", (1, 4, 256, 12, 20), 8, 256, 0.1, 0.1, 0),
    # 600 and 575 keys: the chunked kernels; 575 = 256 + 256 + 63: a ragged last chunk; N = 1725: 108 query tiles, no multiple of 4 * kSpQT
    ("full", (1, 2, 256, 24, 25), 8, 256, 0.1, 0.3, 0),
    ("full", (1, 3, 256, 25, 23), 8, 256, 0.0, 0.1, 0),
    # the VALU kernels (head_dim 8; head_dim 32 under train_valu): they share the index helpers
    ("full", (2, 3, 64, 7, 9), 8, 128, 0.1, 0.1, 0),
    ("axial", (2, 2, 256, 16, 5), 8, 256, 0.3, 0.1, 1),
]
CC_CASE = "g13_cc_train_B2_Q8_Tc2_V1_H4_L1"      # its sizes and weights: the cross-clip module in train() (attn_drop 0.1): passes without `pos`, few sequences


def sha(x):
    return hashlib.sha256(x.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def report(tag, tensors):
    for k, v in tensors:
        print(f"{tag} {k} {sha(v)}", flush=True)


def layer_case(kind, shape, heads, F, p_drop, p_attn, valu):
    B, T, C, H, W = shape
    shapes = orc.axial_layer_param_shapes(C, F)
    if kind == "full":
        shapes = {k.replace("height_attn", "temporal_attn"): v for k, v in shapes.items() if "width_attn" not in k}
    cls = ax.TemporalAxialTrajectoryAttentionLayer if kind == "axial" else ax.TemporalTrajectoryAttentionLayer
    layer = cls(C, F, dropout=p_drop, attn_drop=p_attn, n_heads=heads)
    layer.load_state_dict(orc.random_weights(shapes, 71), strict=True)
    layer = layer.cuda().train()
    layer.dropout_seed = 31337
    src, pos = orc.synthetic_clip(B, T, C, H, W, 71)
    d_out = torch.randn(B * T, H * W, C, generator=torch.Generator().manual_seed(72))
    s, p = src.float().cuda().requires_grad_(True), pos.float().cuda().requires_grad_(True)
    _lib.check(_lib.lib().axvs_set_option(b"train_valu", valu), "axvs_set_option")
    try:
        out = layer(s, p)[0]
        out.backward(d_out.cuda())
        torch.cuda.synchronize()
    finally:
        _lib.lib().axvs_set_option(b"train_valu", 0)
    tag = f"{kind}{list(shape)}h{heads}f{F}p{p_drop}/{p_attn}" + ("valu" if valu else "")
    report(tag, [("out", out), ("d_src", s.grad), ("d_pos", p.grad)] + [("grad." + k, v.grad) for k, v in layer.named_parameters()])


def cc_case(name):
    z = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    m = json.loads(bytes(z["meta"]).decode())
    mod = ax.CrossClipTrackingModule(num_layers=m["layers"], num_classes=m["num_classes"], attn_drop=0.1, aspp_drop=m["p_aspp_drop"],
                                     kernel_sizes=[3, 3, 3], atrous_rates=[1, 2, 3], norm_fn="ln", num_clip_frames=m["V"])
    sd = mod.state_dict()
    sd.update(orc.random_weights({k: tuple(v) for k, v in m["shapes"].items()}, m["seed"]))
    mod.load_state_dict(sd, strict=True)
    mod = mod.cuda().train()
    mod.dropout_seed = m["dropout_seed"]
    g = torch.Generator().manual_seed(m["seed"] + 1)
    cq = torch.randn(m["B"], m["Q"], m["Tc"], 256, generator=g)
    pf = torch.nn.functional.normalize(torch.randn(m["B"], 128, m["Tc"] * m["V"], m["H"], m["W"], generator=g), dim=1)
    q = cq.cuda().requires_grad_(True)
    out = mod(q, pf.cuda())
    logits = torch.stack([a["pred_logits"] for a in out["aux_outputs"]] + [out["pred_logits"]])
    masks = torch.stack([a["pred_masks"] for a in out["aux_outputs"]] + [out["pred_masks"]])
    gl = torch.randn(logits.shape, generator=g).cuda()
    gm = torch.randn(masks.shape, generator=g).cuda()
    ((logits * gl).sum() + (masks * gm).sum()).backward()
    torch.cuda.synchronize()
    report(name, [("logits", logits), ("masks", masks), ("d_clip_query", q.grad)] + [("grad." + k, v.grad) for k, v in mod.named_parameters()])


if __name__ == "__main__":
    for c in CASES:
        layer_case(*c)
    cc_case(CC_CASE)
