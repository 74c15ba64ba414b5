"""Bit record of the device pieces that exist once (csrc/axvs_layout.h, the class heads' shared body in csrc/axvs_cc.h): fixed cases that
between them reach the NCHW <-> rows pair at every call site, the class-logit and broadcast row kernels, both class heads and the
register-resident contraction of the two mask products, one SHA-256 per returned tensor.  Two libraries compute the same bits iff their
outputs are the same text:

    AXVS_LIB_PATH=tools/ab/parent.so python3 tools/device_pieces_bits.py > a.txt;  python3 tools/device_pieces_bits.py > b.txt;  cmp a.txt b.txt
"""
import hashlib, os, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import axial_vs_amd as ax
import convnext_cases as cc
import kmax_decoder_cases as kc
import kmax_pixel_decoder_cases as pc
import m2f_decoder_cases as mc
from golden_util import load, weights

KMAX = ("b", "c", "e")                # odd maps with T 3 / three stacked clips / C 2048 on 2 x 3 with L 256
M2F = ("b", "d", "f")                 # ragged maps / N 3, T 1 / the all-masked rule
KPIX = ("A", "C")                     # maps 3x4 .. 17x25 / 2x6 .. 9x41 with a shortcut conv
CNX = min(cc.NETS, key=lambda c: c.size[0] * c.size[1] * c.N * sum(c.depths))
GLUE = [(2, 64, 256, 5, 7, "in"), (3, 256, 96, 9, 8, "out")]


def sha(x):
    return hashlib.sha256(x.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def report(tag, tensors):
    for k, v in tensors:
        print(f"{tag} {k} {sha(v)}", flush=True)


def kmax(name):
    case = kc.BY_NAME[name]
    dec = ax.KMaXTransformerDecoder(case.dec_layers, case.in_channels, case.K, case.L, case.T, case.B > 1)
    dec.load_state_dict(kc.make_params(case), strict=True)
    x, pan = kc.make_inputs(case)
    out = dec.cuda().eval()([t.float().cuda() for t in x], pan.float().cuda(), return_index_maps=True)
    report(f"kmax_decoder[{name}]", [(k, out[k]) for k in kc.OUTPUTS] + [(f"index_map{i}", m) for i, m in enumerate(out["index_maps"])])


def decoder_cfg(layers):
    """tests/test_hip_m2f_decoder.py's: post-norm layers of cross-attention, self-attention, FFN"""
    lay = dict(type="DetrTransformerDecoderLayer",
               attn_cfgs=dict(type="MultiheadAttention", embed_dims=256, num_heads=8, attn_drop=0.0, proj_drop=0.0, dropout_layer=None, batch_first=False),
               ffn_cfgs=dict(embed_dims=256, feedforward_channels=2048, num_fcs=2, act_cfg=dict(type="ReLU", inplace=True), ffn_drop=0.0,
                             dropout_layer=None, add_identity=True),
               feedforward_channels=2048, operation_order=("cross_attn", "norm", "self_attn", "norm", "ffn", "norm"))
    return dict(type="DetrTransformerDecoder", return_intermediate=True, num_layers=layers, transformerlayers=lay, init_cfg=None)


def m2f(name):
    case = mc.BY_NAME[name]
    dec = ax.TubeLinkClipDecoder(case.Q, case.K, feat_channels=256, out_channels=256, transformer_decoder=decoder_cfg(case.layers),
                                 positional_encoding=dict(type="SinePositionalEncoding3D", num_feats=128, normalize=True), num_transformer_feat_level=3)
    dec.load_state_dict(mc.make_params(case), strict=True)
    mf, mems = mc.make_inputs(case)
    q, cls, mp, lm = dec.cuda()(mf.float().cuda(), [m.float().cuda() for m in mems], return_predictions=True, return_masks=True)
    report(f"m2f_decoder[{name}]", [("query_feat", q), ("cls_pred", cls), ("mask_pred", mp)]
           + [(f"layer{i}.{w}", v) for i, bf in enumerate(lm) for w, v in zip(("bits", "flags"), bf)])


def kpix(name):
    case = pc.BY_NAME[name]
    dec = ax.KMaXPixelDecoder(pc.input_shape(case), case.dec_layers, case.dec_channels, case.layer_types, case.spatial or (64, 64))
    dec.load_state_dict(pc.make_params(case), strict=True)
    feats = {k: v.float().cuda() for k, v in pc.make_inputs(case).items()}
    pan, _, ms = dec.cuda().eval().forward_features(feats)
    report(f"kmax_pixel_decoder[{name}]", list(zip(pc.OUTPUTS, list(ms) + [pan])))


def convnext(case):
    kw = dict(depths=case.depths, dims=case.dims, out_features=cc.OUTPUTS)
    net = ax.ConvNeXtV2Backbone(**kw) if case.v2 else ax.ConvNeXtBackbone(layer_scale_init_value=1e-6 if case.gamma else 0.0, **kw)
    net.load_state_dict(cc.net_params(case), strict=True)
    outs = net.cuda().eval()(cc.net_input(case).float().cuda())
    report(f"convnext[{case.name}]", [(k, outs[k]) for k in cc.OUTPUTS])


def cc_module(name):
    z, m = load(name)
    g = torch.Generator().manual_seed(m["seed"] + 1)
    cq = torch.randn(m["B"], m["Q"], m["Tc"], 256, generator=g)
    pf = torch.nn.functional.normalize(torch.randn(m["B"], 128, m["Tc"] * m["V"], m["H"], m["W"], generator=g), dim=1)
    mod = ax.CrossClipTrackingModule(num_layers=m["layers"], num_classes=m["num_classes"], attn_drop=0.0, aspp_drop=0.0, kernel_sizes=[3, 3, 3],
                                     atrous_rates=[1, 2, 3], norm_fn=m.get("norm_fn", "ln"), num_clip_frames=m["V"]).eval()
    sd = mod.state_dict()
    sd.update(weights(z, m))
    mod.load_state_dict(sd, strict=True)
    out = mod.cuda()(cq.cuda(), pf.cuda())
    heads = out["aux_outputs"] + [out]
    report(name, [(f"layer{i}.{k}", h[k]) for i, h in enumerate(heads) for k in ("pred_logits", "pred_masks")])


def tl_head(name):
    z, m = load(name)
    g = torch.Generator().manual_seed(m["seed"] + 1)
    cq = torch.randn(m["B"], m["Tc"], m["Q"], 256, generator=g)
    mf = torch.nn.functional.normalize(torch.randn(m["B"], m["Tc"] * m["fpc"], m["Cm"], m["h"], m["w"], generator=g), dim=2)
    mod = ax.TubeLinkCrossClipHead(num_classes=m["num_classes"], out_channels=m["Cm"], num_cc_layers=m["layers"]).eval()
    mod.load_state_dict(weights(z, m), strict=True)
    cls, masks = mod.cuda()(cq.cuda(), mf.cuda())
    report(name, [(f"layer{i}.cls", c) for i, c in enumerate(cls)] + [(f"layer{i}.masks", x) for i, x in enumerate(masks)])


def glue(N, Cin, Cout, H, W, direction):
    """tests/test_hip_glue_training.py's data: "in" = an NCHW map to token rows (and its gradient back), "out" the other way"""
    from axial_vs_amd.glue_training import conv_gn_train
    g = torch.Generator().manual_seed(1000 + Cin + H)
    conv, gn = torch.nn.Conv2d(Cin, Cout, 1), torch.nn.GroupNorm(32, Cout)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * (1.5 / Cin ** 0.5))
        conv.bias.copy_(torch.randn(Cout, generator=g) * 0.3)
        gn.weight.copy_(torch.rand(Cout, generator=g) + 0.5)
        gn.bias.copy_(torch.randn(Cout, generator=g) * 0.2)
    x = torch.randn(N, Cin, H, W, generator=g) * 1.3 + 0.2
    d_out = torch.randn(N, Cout, H, W, generator=g)
    conv, gn = conv.cuda(), gn.cuda()
    if direction == "in":
        xg = x.cuda().requires_grad_(True)
        out = conv_gn_train(xg, conv, gn, out_layout="tokens")
        out.backward(d_out.flatten(2).transpose(1, 2).contiguous().cuda())
    else:
        xg = x.flatten(2).transpose(1, 2).contiguous().cuda().requires_grad_(True)
        out = conv_gn_train(xg, conv, gn, out_layout="nchw", hw=(H, W))
        out.backward(d_out.cuda())
    torch.cuda.synchronize()
    report(f"conv1x1_gn_train{(N, Cin, Cout, H, W, direction)}", [("out", out), ("d_x", xg.grad), ("d_conv_w", conv.weight.grad), ("d_conv_b", conv.bias.grad),
                                                                    ("d_gn_w", gn.weight.grad), ("d_gn_b", gn.bias.grad)])


if __name__ == "__main__":
    with torch.no_grad():
        for n in KMAX:
            kmax(n)
        for n in M2F:
            m2f(n)
        for n in KPIX:
            kpix(n)
        convnext(CNX)
        cc_module("g5_cc_module_Q16_Tc3_V2_H8_L2")
        tl_head("g6_tl_cc_head_Tc3_Q16_f2_L2")
    for c in GLUE:
        glue(*c)
