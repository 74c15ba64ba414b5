"""Cases and restatement of Tube-Link's per-clip masked-attention query decoder (axial_vs_amd.TubeLinkClipDecoder).

`Restatement` states the semantics once, in the reference's op order (MaXTron_Tube-Link/models/video/tube_link_vis/
mask2former_video_cc_head.py:840-903 with forward_head_video :738-759, under mmcv 1.6.1's DetrTransformerDecoderLayer): the mask head
computes the full-resolution einsum, THEN F.interpolate, THEN the threshold.  It runs in float64 (the yardstick) or float32 (whose own
error against float64 sizes every bound of the tests: band and tolerance are 8 x that error, this project's standing factor).

One departure, immaterial in float64: the reference thresholds `sigmoid(logit) < 0.5`; here `logit < 0` (the two differ only where
|logit| is below the rounding of 0.5, ~1e-16 in float64 and ~6e-8 in float32, far inside every band).
"""
from collections import OrderedDict, namedtuple
import math

import torch
import torch.nn.functional as F

C, HEADS, FFN = 256, 8, 2048

Case = namedtuple("Case", "name seed N Q T hw levels layers K boost")
# boost: scale of row 0 of the last mask_embed layer, with channel 0 of the mask features constant 1 -- a per-query offset on all of a
# query's logits, so that some queries have every key masked and some none (case f)
CASES = [
    Case("a", 101, 1, 100, 2, (24, 40), ((3, 5), (6, 10), (12, 20)), 9, 40, 0.0),       # baseline
    Case("b", 202, 1, 100, 2, (25, 38), ((4, 5), (7, 10), (13, 19)), 9, 40, 0.0),       # ragged: non-integer ratios, keys 40 / 140 / 494
    Case("c", 303, 1, 8, 3, (10, 14), ((2, 3), (3, 5), (5, 7)), 3, 5, 0.0),             # small Q, odd T
    Case("d", 404, 3, 20, 1, (12, 16), ((2, 2), (3, 4), (6, 8)), 3, 7, 0.0),            # N = 3, T = 1
    Case("e", 505, 1, 100, 2, (20, 26), ((3, 4), (5, 7), (13, 23)), 3, 40, 0.0),        # key split: 598 keys = 3 chunks of 224, the last partial
    Case("f", 606, 2, 24, 2, (12, 16), ((2, 3), (3, 4), (6, 8)), 3, 7, 40.0),           # the all-masked rule
]
# fixtures of the reference's own classes (tools/gen_golden_m2f_decoder.py; the stored seed is the first without a flipped bit): one
# video of N = 2 clips
FIXTURES = [
    Case("g23_m2f_Q16_T2_L3", 2300, 2, 16, 2, (12, 20), ((2, 3), (3, 5), (6, 10)), 3, 7, 0.0),
    Case("g23_m2f_Q100_T2_L9", 2310, 2, 100, 2, (24, 40), ((3, 5), (6, 10), (12, 20)), 9, 40, 0.0),
]
# cases whose fp32 free run agrees with float64 in every bit (test_case_screening asserts it): the end-to-end numbers compare there.
# The issue asks it of a, c and f; the seeds of b, d and e give it too, and it is recorded here so that a change of seed cannot
# switch their end-to-end assertions off unnoticed.
NO_FLIP = ("a", "b", "c", "d", "e", "f")
BY_NAME = {c.name: c for c in CASES}


def keys_of(case, level):
    return case.T * case.levels[level][0] * case.levels[level][1]


def param_shapes(Q, K1, layers):
    """state-dict keys of the decoder (the head's own names) -> shapes"""
    s = OrderedDict()
    for i in range(layers):
        p = f"transformer_decoder.layers.{i}."
        for a in (0, 1):
            s[p + f"attentions.{a}.attn.in_proj_weight"] = (3 * C, C)
            s[p + f"attentions.{a}.attn.in_proj_bias"] = (3 * C,)
            s[p + f"attentions.{a}.attn.out_proj.weight"] = (C, C)
            s[p + f"attentions.{a}.attn.out_proj.bias"] = (C,)
        s[p + "ffns.0.layers.0.0.weight"] = (FFN, C)
        s[p + "ffns.0.layers.0.0.bias"] = (FFN,)
        s[p + "ffns.0.layers.1.weight"] = (C, FFN)
        s[p + "ffns.0.layers.1.bias"] = (C,)
        for n in range(3):
            s[p + f"norms.{n}.weight"] = (C,)
            s[p + f"norms.{n}.bias"] = (C,)
    s["transformer_decoder.post_norm.weight"] = (C,)
    s["transformer_decoder.post_norm.bias"] = (C,)
    s["query_embed.weight"] = (Q, C)
    s["query_feat.weight"] = (Q, C)
    s["level_embed.weight"] = (3, C)
    s["cls_embed.weight"] = (K1, C)
    s["cls_embed.bias"] = (K1,)
    for n in (0, 2, 4):
        s[f"mask_embed.{n}.weight"] = (C, C)
        s[f"mask_embed.{n}.bias"] = (C,)
    return s


def make_params(case, seed=None):
    """fp32-representable values: xavier-uniform matrices, biases U(-0.1, 0.1), norm gains 1 + U(-0.1, 0.1), N(0, 1) embeddings"""
    g = torch.Generator().manual_seed(case.seed if seed is None else seed)
    out = OrderedDict()
    for k, shp in param_shapes(case.Q, case.K + 1, case.layers).items():
        if k.split(".")[0] in ("query_embed", "query_feat", "level_embed"):
            v = torch.randn(shp, generator=g)
        elif len(shp) == 2:
            v = (torch.rand(shp, generator=g) * 2 - 1) * math.sqrt(6.0 / (shp[0] + shp[1]))
        elif "norm" in k and k.endswith("weight"):
            v = 1.0 + (torch.rand(shp, generator=g) * 2 - 1) * 0.1
        else:
            v = (torch.rand(shp, generator=g) * 2 - 1) * 0.1
        out[k] = v.float()
    if case.boost:
        out["mask_embed.4.weight"][0] *= case.boost
    return out


def make_inputs(case, seed=None):
    """(mask_features [N,T,C,h,w], [three memories [N,T,C,h_l,w_l]]) fp32, N(0, 1)"""
    g = torch.Generator().manual_seed((case.seed if seed is None else seed) + 1)
    mf = torch.randn(case.N, case.T, C, *case.hw, generator=g)
    if case.boost:
        mf[:, :, 0] = 1.0
    mems = [torch.randn(case.N, case.T, C, *s, generator=g) for s in case.levels]
    return mf, mems


def sine3d(T, H, W, dtype, num_feats=128, temperature=10000.0, scale=2 * math.pi, eps=1e-6, device=None):
    """SinePositionalEncoding3D(num_feats, normalize=True) on an all-valid mask -> [T, 2 num_feats, H, W]
    (tube_link_vps/position_encoding.py:55-99), built with torch ops on `device` as the reference builds it on its mask's device"""
    z = torch.arange(1, T + 1, dtype=dtype, device=device)[:, None, None].expand(T, H, W)
    y = torch.arange(1, H + 1, dtype=dtype, device=device)[None, :, None].expand(T, H, W)
    x = torch.arange(1, W + 1, dtype=dtype, device=device)[None, None, :].expand(T, H, W)
    z, y, x = z / (T + eps) * scale, y / (H + eps) * scale, x / (W + eps) * scale
    dim_t = torch.arange(num_feats, dtype=dtype, device=device)
    dim_t = temperature ** (2 * torch.div(dim_t, 2, rounding_mode="floor") / num_feats)
    dim_z = torch.arange(2 * num_feats, dtype=dtype, device=device)
    dim_z = temperature ** (2 * torch.div(dim_z, 2, rounding_mode="floor") / (2 * num_feats))
    px, py, pz = x[..., None] / dim_t, y[..., None] / dim_t, z[..., None] / dim_z
    px = torch.stack((px[..., 0::2].sin(), px[..., 1::2].cos()), dim=4).flatten(3)
    py = torch.stack((py[..., 0::2].sin(), py[..., 1::2].cos()), dim=4).flatten(3)
    pz = torch.stack((pz[..., 0::2].sin(), pz[..., 1::2].cos()), dim=4).flatten(3)
    return (torch.cat((py, px), dim=3) + pz).permute(0, 3, 1, 2)


class Restatement:
    """The decoder in `dtype`.  Queries travel as [Q, N, C] (the reference's layout)."""

    def __init__(self, params, mask_features, memories, dtype, layers):
        self.p = {k: v.to(dtype) for k, v in params.items()}
        self.dtype, self.layers = dtype, layers
        self.mf = mask_features.to(dtype)
        self.N, self.T = self.mf.shape[:2]
        self.sizes = [tuple(m.shape[-2:]) for m in memories]
        lvl = self.p["level_embed.weight"]
        self.values, self.pos = [], []
        for l, m in enumerate(memories):          # (t, y, x) token order, :851-859
            self.values.append(m.to(dtype).flatten(3).permute(1, 3, 0, 2).flatten(0, 1) + lvl[l].view(1, 1, -1))
            pe = sine3d(self.T, *self.sizes[l], dtype, device=self.mf.device)[None].expand(self.N, -1, -1, -1, -1)
            self.pos.append(pe.flatten(3).permute(1, 3, 0, 2).flatten(0, 1))
        self.query_pos = self.p["query_embed.weight"][:, None].repeat(1, self.N, 1)

    def start(self):
        return self.p["query_feat.weight"][:, None].repeat(1, self.N, 1)

    def _ln(self, x, name):
        return F.layer_norm(x, (C,), self.p[name + ".weight"], self.p[name + ".bias"], 1e-5)

    def mask_embed(self, x):
        """post_norm -> [N,Q,C] -> (post-normed queries, mask_embed MLP)"""
        y = self._ln(x, "transformer_decoder.post_norm").transpose(0, 1)
        m = y
        for n in (0, 2, 4):
            m = F.linear(m, self.p[f"mask_embed.{n}.weight"], self.p[f"mask_embed.{n}.bias"])
            if n != 4:
                m = F.relu(m)
        return y, m

    def predictions(self, x):
        y, m = self.mask_embed(x)
        return F.linear(y, self.p["cls_embed.weight"], self.p["cls_embed.bias"]), torch.einsum("bqc,btchw->btqhw", m, self.mf)

    def head_logits(self, x, level):
        """forward_head_video's attention logits [N, Q, T*h_l*w_l], the reference's order: einsum at full resolution, then the resize"""
        _, mask_pred = self.predictions(x)
        am = F.interpolate(mask_pred.flatten(0, 1), self.sizes[level], mode="bilinear", align_corners=False).unflatten(0, (self.N, self.T))
        return am.flatten(3).transpose(1, 2).flatten(2)

    def head_logits_level(self, x, level):
        """the same logits in the level-resolution form: mask_embed . resize(mask_feature)"""
        _, m = self.mask_embed(x)
        r = F.interpolate(self.mf.flatten(0, 1), self.sizes[level], mode="bilinear", align_corners=False).unflatten(0, (self.N, self.T))
        return torch.einsum("bqc,btchw->btqhw", m, r).flatten(3).transpose(1, 2).flatten(2)

    def _attn(self, i, a, query, key, value, query_pos, key_pos, mask):
        """mmcv's MultiheadAttention wrapper around nn.MultiheadAttention: positions on query and key, identity = query, no dropout"""
        p = f"transformer_decoder.layers.{i}.attentions.{a}.attn."
        out = F.multi_head_attention_forward(query + query_pos, key + key_pos, value, C, HEADS, self.p[p + "in_proj_weight"], self.p[p + "in_proj_bias"],
                                             None, None, False, 0.0, self.p[p + "out_proj.weight"], self.p[p + "out_proj.bias"], training=False,
                                             need_weights=False, attn_mask=mask)[0]
        return query + out

    def layer(self, i, x, masked):
        """layer i on queries x [Q,N,C] with `masked` bool [N,Q,S] (True = key masked) as the mask head gave it: a row that is all True
        is set all False first (:879-880)"""
        level = i % 3
        masked = masked.clone()
        masked[masked.all(dim=-1)] = False
        am = masked.unsqueeze(1).repeat(1, HEADS, 1, 1).flatten(0, 1)
        p = f"transformer_decoder.layers.{i}."
        x = self._ln(self._attn(i, 0, x, self.values[level], self.values[level], self.query_pos, self.pos[level], am), p + "norms.0")
        x = self._ln(self._attn(i, 1, x, x, x, self.query_pos, self.query_pos, None), p + "norms.1")
        h = F.relu(F.linear(x, self.p[p + "ffns.0.layers.0.0.weight"], self.p[p + "ffns.0.layers.0.0.bias"]))
        x = x + F.linear(h, self.p[p + "ffns.0.layers.1.weight"], self.p[p + "ffns.0.layers.1.bias"])
        return self._ln(x, p + "norms.2")

    def run(self):
        """free run -> per layer dict(x_in, logits, x_out) and the last layer's output"""
        x, rec = self.start(), []
        for i in range(self.layers):
            logits = self.head_logits(x, i % 3)
            out = self.layer(i, x, logits < 0)
            rec.append(dict(x_in=x, logits=logits, x_out=out))
            x = out
        return rec, x


_CACHE = {}


def study(case):
    """Everything the tests of one case share, computed once and left unchanged: float64 and fp32 free runs, the fp32 restatement
    teacher-forced on the float64 chain, the bands and tolerances."""
    if case.name in _CACHE:
        return _CACHE[case.name]
    with torch.no_grad():
        params = make_params(case)
        mf, mems = make_inputs(case)
        r64 = Restatement(params, mf, mems, torch.float64, case.layers)
        r32 = Restatement(params, mf, mems, torch.float32, case.layers)
        rec64, out64 = r64.run()
        rec32, out32 = r32.run()
        layers = []
        for i in range(case.layers):
            a, b = rec64[i], rec32[i]
            x32 = a["x_in"].float()
            tf_logits = r32.head_logits(x32, i % 3).double()
            tf_out = r32.layer(i, x32, a["logits"] < 0).double()
            layers.append(dict(
                x_in=a["x_in"], logits=a["logits"], masked=a["logits"] < 0, x_out=a["x_out"],
                band_tf=8 * float((tf_logits - a["logits"]).abs().max()),                    # mask head, teacher-forced
                tol_layer=8 * float((tf_out - a["x_out"]).abs().max()),                      # layer, teacher-forced
                band_free=8 * float((b["logits"].double() - a["logits"]).abs().max()),       # free run
                flips32=int(((b["logits"] < 0) != (a["logits"] < 0)).sum())))
        cls64, mp64 = r64.predictions(out64)
        cls32, mp32 = r32.predictions(out32)
        st = dict(case=case, params=params, mf=mf, mems=mems, r64=r64, r32=r32, layers=layers, out=out64,
                  tol_out=8 * float((out32.double() - out64).abs().max()), cls=cls64, mask_pred=mp64,
                  tol_cls=8 * float((cls32.double() - cls64).abs().max()), tol_mask=8 * float((mp32.double() - mp64).abs().max()))
    _CACHE[case.name] = st
    return st
