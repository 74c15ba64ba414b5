"""Cases and restatement of Video-kMaX's k-means query decoder (axial_vs_amd.KMaXTransformerDecoder).

`Restatement` states the eval forward once, in the reference's op order (MaXTron_Video-kMaX/maxtron_deeplab/modeling/transformer_decoder/
maxtron_transformer_decoder.py:49-231, 416-590): every norm is F.batch_norm on its running statistics (eps 1e-3), the mask logits are
built in full, the argmax is `max(1)`, the one-hot tensor is scattered and contracted with the pixel values.  It runs in float64 (the
yardstick) or float32, whose own error against float64 sizes every bound of the tests: band and tolerance are 8 x that error, this
project's standing factor.  Queries travel as [B, 256, L], the reference's layout.

The argmax is a hard decision, so the cases are screened (test_kmax_decoder_cpu.py::test_case_screening): the stored seed of a case is the
first whose float32 run takes every decision of the float64 run and whose closest top-two margin is outside 8 x the float32 logit error.
"""
from collections import OrderedDict, namedtuple
import math

import torch
import torch.nn.functional as F

EPS = 1e-3
Case = namedtuple("Case", "name seed L K T levels pan in_channels dec_layers B mask_gain")
# K classes (K + 1 logits); B > 1 runs through cross_clip_training with num_clip_frames = T
CASES = [
    Case("a", 101, 128, 7, 2, ((3, 5), (6, 10), (12, 20)), (24, 40), (96, 64, 32), (2, 2, 2), 1, 0.1),       # baseline
    Case("b", 200, 100, 124, 3, ((4, 5), (7, 10), (13, 19)), (25, 38), (64, 48, 32), (2, 2, 2), 1, 0.1),     # ragged: L, K1, odd maps, T 3
    Case("c", 300, 20, 4, 1, ((2, 3), (4, 5), (7, 9)), (14, 18), (32, 32, 16), (1, 1, 1), 3, 0.1),           # three stacked clips of one frame
    Case("d", 400, 128, 7, 2, ((3, 5), (6, 10), (12, 20)), (24, 40), (96, 64, 32), (2, 2, 2), 1, -0.1),      # case a, the mask norm's gain negative
    Case("e", 500, 256, 3, 2, ((2, 3), (3, 4), (5, 6)), (9, 11), (2048, 32, 16), (1, 1, 1), 1, 0.1),         # L 256 (four LDS chunks), contraction 2048
    Case("f", 600, 24, 5, 2, ((3, 4), (5, 8), (10, 16)), (20, 32), (32, 32, 16), (1, 1, 1), 1, 0.1),         # h 3: a window over frame edge and map edge
    Case("g", 700, 24, 5, 3, ((2, 4), (4, 8), (8, 16)), (16, 32), (32, 32, 16), (1, 1, 1), 1, 0.1),          # h 2, T 3: a window over two frame edges
]
# fixtures of the reference's own classes (tools/gen_golden_kmax_decoder.py writes the seed it kept into the file)
FIXTURES = [
    Case("g24_kmax_L16_T2", 2400, 16, 4, 2, ((2, 3), (4, 6), (8, 12)), (16, 24), (32, 32, 16), (1, 1, 1), 2, 0.1),
    Case("g24_kmax_L100_T2", 2410, 100, 18, 2, ((3, 5), (6, 10), (12, 20)), (24, 40), (64, 48, 32), (2, 2, 2), 1, 0.1),
]
BY_NAME = {c.name: c for c in CASES}


def layer_levels(case):
    return [l for l, n in enumerate(case.dec_layers) for _ in range(n)]


def _convbn(s, p, cout, cin, k=(), bias=False, norm=True):
    s[p + "conv.weight"] = (cout, cin) + tuple(k)
    if bias:
        s[p + "conv.bias"] = (cout,)
    if norm:
        _bn(s, p + "norm.", cout)


def _bn(s, p, c):
    s[p + "weight"], s[p + "bias"], s[p + "running_mean"], s[p + "running_var"], s[p + "num_batches_tracked"] = (c,), (c,), (c,), (c,), ()


def _predictor(s, p, K1):
    _convbn(s, p + "_pixel_space_head_conv0bnact.", 256, 1, (5, 5))
    _convbn(s, p + "_pixel_space_head_conv1bnact.", 256, 256, (1, 1))
    _convbn(s, p + "_pixel_space_head_last_convbn.", 128, 256, (1, 1), bias=True)
    _convbn(s, p + "_transformer_mask_head.", 128, 256, (1,))
    _convbn(s, p + "_transformer_class_head.", K1, 256, (1,), bias=True, norm=False)
    _bn(s, p + "_pixel_space_mask_batch_norm.", 1)


def param_shapes(case):
    """state-dict keys of the decoder (the reference's own names, in its registration order) -> shapes"""
    s, K1 = OrderedDict(), case.K + 1
    for i, l in enumerate(layer_levels(case)):
        p = f"_kmax_transformer_layers.{i}."
        _convbn(s, p + "_query_conv1_bn_act.", 256, 256, (1,))
        _convbn(s, p + "_pixel_conv1_bn_act.", 256, case.in_channels[l], (1, 1))
        _convbn(s, p + "_query_qkv_conv_bn.", 512, 256, (1,))
        _convbn(s, p + "_pixel_v_conv_bn.", 256, 256, (1, 1))
        _bn(s, p + "_query_self_attention._batch_norm_similarity.", 8)
        _bn(s, p + "_query_self_attention._batch_norm_retrieved_value.", 256)
        _convbn(s, p + "_query_conv3_bn.", 256, 256, (1,))
        _convbn(s, p + "_query_ffn_conv1_bn_act.", 2048, 256, (1,))
        _convbn(s, p + "_query_ffn_conv2_bn.", 256, 2048, (1,))
        _predictor(s, p + "_predictor.", K1)
        _bn(s, p + "_kmeans_query_batch_norm_retrieved_value.", 256)
        _convbn(s, p + "_kmeans_query_conv3_bn.", 256, 256, (1,))
    s["_cluster_centers.weight"] = (256, case.L)
    _convbn(s, "_class_embedding_projection.", 256, 256, (1,))
    _convbn(s, "_mask_embedding_projection.", 256, 256, (1,))
    _predictor(s, "_predictor.", K1)
    return s


def make_params(case, seed=None):
    """fp32 values: xavier-uniform convolutions, biases and running means U(-0.1, 0.1), running variances U(0.5, 1.5), gains
    1 + U(-0.1, 0.1) (not the reference's zero norm_init: every update counts), the mask norm's gain `case.mask_gain`, N(0, 1) centers"""
    g = torch.Generator().manual_seed(case.seed if seed is None else seed)
    out = OrderedDict()
    u = lambda shp: torch.rand(shp, generator=g) * 2 - 1
    for k, shp in param_shapes(case).items():
        if k.endswith("num_batches_tracked"):
            v = torch.tensor(0, dtype=torch.long)
        elif k == "_cluster_centers.weight":
            v = torch.randn(shp, generator=g)
        elif k.endswith("conv.weight"):
            fan = math.prod(shp[2:])
            v = u(shp) * math.sqrt(6.0 / (shp[0] * fan / (1 if shp[1] > 1 else shp[0]) + shp[1] * fan))
        elif k.endswith("running_var"):
            v = 1.0 + 0.5 * u(shp)
        elif k.endswith("_pixel_space_mask_batch_norm.weight"):
            v = torch.full(shp, case.mask_gain)
        elif k.endswith("norm.weight") or k.endswith("_value.weight") or k.endswith("_similarity.weight"):
            v = 1.0 + 0.1 * u(shp)
        else:
            v = 0.1 * u(shp)
        out[k] = v if v.dtype == torch.long else v.float()
    return out


def make_inputs(case, seed=None):
    """(three levels [(B T), C_l, h_l, w_l], panoptic features [(B T), 256, H, W]) fp32, N(0, 1)"""
    g = torch.Generator().manual_seed((case.seed if seed is None else seed) + 1)
    BT = case.B * case.T
    x = [torch.randn(BT, c, *s, generator=g) for c, s in zip(case.in_channels, case.levels)]
    return x, torch.randn(BT, 256, *case.pan, generator=g)


def stack(t, B):
    """(b t) c h w -> b c (t h) w"""
    BT, c, h, w = t.shape
    return t.view(B, BT // B, c, h, w).permute(0, 2, 1, 3, 4).reshape(B, c, BT // B * h, w)


class Restatement:
    """The decoder's eval forward in `dtype`."""

    def __init__(self, params, case, dtype):
        self.p = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in params.items()}
        self.case, self.dtype = case, dtype

    def softmax(self, sim):
        """the query self-attention's softmax over the keys: a method, so that a test can record its scores or state it wrongly"""
        return F.softmax(sim, dim=-1)

    def bn(self, x, p):
        q = self.p
        return F.batch_norm(x, q[p + "running_mean"], q[p + "running_var"], q[p + "weight"], q[p + "bias"], False, 0.01, EPS)

    def convbn(self, x, p, act=False, **kw):
        w = self.p[p + "conv.weight"]
        x = (F.conv1d if w.dim() == 3 else F.conv2d)(x, w, self.p.get(p + "conv.bias"), **kw)
        if p + "norm.weight" in self.p:
            x = self.bn(x, p + "norm.")
        return F.gelu(x) if act else x

    def predictor(self, p, mask_embeddings, class_embeddings, pixel_feature):
        """kMaXPredictor.forward: pixel_feature [B, C, TH, W] -- the depthwise window runs over the stacked map"""
        f = self.convbn(pixel_feature, p + "_pixel_space_head_conv0bnact.", True, padding=2, groups=pixel_feature.shape[1])
        f = self.convbn(f, p + "_pixel_space_head_conv1bnact.", True)
        f = self.convbn(f, p + "_pixel_space_head_last_convbn.")
        f = F.normalize(f, p=2, dim=1)
        cls = self.convbn(class_embeddings, p + "_transformer_class_head.").permute(0, 2, 1).contiguous()
        bias = [0.0] * cls.shape[-1]
        bias[-1] = math.log((cls.shape[-1] - 1) * 0.9 / (1 - 0.9))
        cls = cls + torch.tensor(bias, dtype=cls.dtype).to(cls)
        kernel = self.convbn(mask_embeddings, p + "_transformer_mask_head.")
        logits = torch.einsum("bchw,bcn->bnhw", f, kernel)
        logits = self.bn(logits.unsqueeze(1), p + "_pixel_space_mask_batch_norm.").squeeze(1)
        return dict(class_logits=cls, mask_logits=logits, mask_embeddings=kernel.permute(0, 2, 1).contiguous(), pixel_feature=f)

    def layer(self, i, pixel_feature, query, index=None):
        """kMaXTransformerLayer.forward on the stacked map [B, C, TH, W] and queries [B, 256, L]; `index` [B, TH*W] given: it stands for
        the argmax.  -> (new queries, prediction result, index used)"""
        p = f"_kmax_transformer_layers.{i}."
        N, L = query.shape[0], query.shape[2]
        pixel_space = self.convbn(F.gelu(pixel_feature), p + "_pixel_conv1_bn_act.", True)
        query_space = self.convbn(query, p + "_query_conv1_bn_act.", True)
        pixel_value = self.convbn(pixel_space, p + "_pixel_v_conv_bn.").reshape(N, 256, -1)
        res = self.predictor(p + "_predictor.", query_space, query_space, pixel_space)
        clustering = res["mask_logits"].flatten(2)
        if index is None:
            index = clustering.max(1, keepdim=True)[1]
        else:
            index = index.long().unsqueeze(1)
        onehot = torch.zeros_like(clustering).scatter_(1, index, 1.0)
        update = torch.einsum("blm,bdm->bdl", onehot, pixel_value)
        update = self.bn(update, p + "_kmeans_query_batch_norm_retrieved_value.")
        update = self.convbn(update, p + "_kmeans_query_conv3_bn.")
        query = query + update
        qkv = self.convbn(query_space, p + "_query_qkv_conv_bn.")
        q, k, v = torch.split(qkv, [128, 128, 256], dim=1)
        q, k, v = q.reshape(N, 8, 16, L), k.reshape(N, 8, 16, L), v.reshape(N, 8, 32, L)
        sim = self.bn(torch.einsum("bhdl,bhdm->bhlm", q, k), p + "_query_self_attention._batch_norm_similarity.")
        got = torch.einsum("bhlm,bhdm->bhdl", self.softmax(sim), v).reshape(N, 256, L)
        got = F.gelu(self.bn(got, p + "_query_self_attention._batch_norm_retrieved_value."))
        query = F.gelu(query + self.convbn(got, p + "_query_conv3_bn."))
        ffn = self.convbn(self.convbn(query, p + "_query_ffn_conv1_bn_act.", True), p + "_query_ffn_conv2_bn.")
        return F.gelu(query + ffn), res, index.squeeze(1)

    def start(self):
        return self.p["_cluster_centers.weight"].unsqueeze(0).repeat(self.case.B, 1, 1)

    def final(self, query, panoptic_features):
        """the projections and the final predictor -> the five outputs"""
        B, T = self.case.B, self.case.T
        res = self.predictor("_predictor.", self.convbn(query, "_mask_embedding_projection.", True),
                             self.convbn(query, "_class_embedding_projection.", True), stack(panoptic_features.to(self.dtype), B))
        unstack = lambda t: t.view(*t.shape[:2], T, t.shape[2] // T, t.shape[3])
        return dict(pred_logits=res["class_logits"], pred_masks=unstack(res["mask_logits"]), pred_mask_embeddings=res["mask_embeddings"],
                    pixel_feature=unstack(res["pixel_feature"]), cluster_centers=query.permute(0, 2, 1).contiguous())

    def run(self, x, panoptic_features):
        """free run -> (per layer dict(q_in, logits [B,L,S], index [B,S], class_logits, q_out), the outputs)"""
        q, rec = self.start(), []
        for i, l in enumerate(layer_levels(self.case)):
            out, res, index = self.layer(i, stack(x[l].to(self.dtype), self.case.B), q)
            rec.append(dict(q_in=q, logits=res["mask_logits"].flatten(2), index=index, class_logits=res["class_logits"], q_out=out))
            q = out
        return rec, self.final(q, panoptic_features)


OUTPUTS = ("pred_logits", "pred_masks", "pred_mask_embeddings", "pixel_feature", "cluster_centers")
_CACHE = {}


def study(case, seed=None):
    """Everything the tests of one case share, computed once and left unchanged: the float64 and float32 free runs, the float32
    restatement teacher-forced on the float64 chain, margins, bands and tolerances."""
    key = (case.name, seed)
    if key in _CACHE:
        return _CACHE[key]
    with torch.no_grad():
        params = make_params(case, seed)
        x, pan = make_inputs(case, seed)
        r64, r32 = Restatement(params, case, torch.float64), Restatement(params, case, torch.float32)
        rec64, out64 = r64.run(x, pan)
        rec32, out32 = r32.run(x, pan)
        layers = []
        for i, l in enumerate(layer_levels(case)):
            a, b = rec64[i], rec32[i]
            tf_out, tf_res, _ = r32.layer(i, stack(x[l], case.B), a["q_in"].float())                      # teacher-forced on the float64 queries
            tf_upd, _, _ = r32.layer(i, stack(x[l], case.B), a["q_in"].float(), index=a["index"])          # ... and on the float64 index map
            top2 = a["logits"].topk(min(2, case.L), dim=1)[0]
            layers.append(dict(
                level=l, q_in=a["q_in"], logits=a["logits"], index=a["index"], q_out=a["q_out"], class_logits=a["class_logits"],
                margin=top2[:, 0] - top2[:, -1] if case.L > 1 else torch.full_like(top2[:, 0], math.inf),       # [B, S]
                band_tf=8 * float((tf_res["mask_logits"].flatten(2).double() - a["logits"]).abs().max()),
                band_free=8 * float((b["logits"].double() - a["logits"]).abs().max()),
                tol_cls=8 * float((tf_res["class_logits"].double() - a["class_logits"]).abs().max()),
                tol_layer=8 * float((tf_upd.double() - a["q_out"]).abs().max()),
                flips_tf=int((tf_res["mask_logits"].flatten(2).max(1)[1] != a["index"]).sum()),
                flips_free=int((b["index"] != a["index"]).sum())))
        st = dict(case=case, params=params, x=x, pan=pan, r64=r64, r32=r32, layers=layers, out=out64, out32=out32,
                  tol={k: 8 * float((out32[k].double() - out64[k]).abs().max()) for k in OUTPUTS})
    _CACHE[key] = st
    return st


def clean(st):
    """the screening condition: no decision of the float32 runs differs, and no top-two margin lies within the 8 x bands"""
    return all(y["flips_tf"] == 0 and y["flips_free"] == 0 and float(y["margin"].min()) > max(y["band_tf"], y["band_free"]) for y in st["layers"])
