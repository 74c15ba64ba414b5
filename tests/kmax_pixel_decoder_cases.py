"""Cases and restatement of Video-kMaX's pixel decoder (axial_vs_amd.KMaXPixelDecoder).

`Restatement` states the eval forward once, in the reference's op order (MaXTron_Video-kMaX/kmax_deeplab/modeling/pixel_decoder/
kmax_pixel_decoder.py:76-371): the three full [N, 8, L, L] similarity tensors concatenated and sent through F.batch_norm on the running
statistics (eps 1e-3), the [L, L, d] relative-position tables built by gather, F.interpolate for the fuses, the channels-first LayerNorm
as the reference writes it.  It runs in float64 (the yardstick) or float32, whose own error against float64 sizes every bound of the
tests: 8 x that error per compared tensor, this project's standing factor (9 x against fixtures of the reference's own fp32 run).
The reference itself cannot run in float64: its softmax casts to float and the next einsum fails on mixed types.

No hard decision is taken anywhere in this decoder, so no case is screened.
"""
from collections import OrderedDict, namedtuple
import math
import types

import torch
import torch.nn.functional as F

EPS = 1e-3
MAX_SPAN = 255
STRIDES = (32, 16, 8, 4)
Case = namedtuple("Case", "name seed spatial N in_channels dec_layers dec_channels layer_types")
_SHIPPED = dict(dec_layers=(1, 5, 1, 1), dec_channels=(512, 256, 128, 64), layer_types=("axial", "axial", "bottleneck", "bottleneck"))
# in_channels: res2 .. res5
CASES = [
    Case("A", 2601, (65, 97), 2, (256, 512, 1024, 2048), **_SHIPPED),        # maps 3x4, 5x7, 9x13, 17x25; align_corners off, on, on
    Case("B", 2602, (64, 96), 1, (256, 512, 1024, 2048), **_SHIPPED),        # maps 2x3, 4x6, 8x12, 16x24; align_corners on, off, off
    Case("C", 2603, (33, 161), 3, (192, 384, 768, 1536), **_SHIPPED),        # maps 2x6, 3x11, 5x21, 9x41; a shortcut conv in stage 0
    Case("D", 2604, (65, 97), 2, (256, 512, 1024, 2048), (2, 1, 2, 2), (512, 256, 128, 64), _SHIPPED["layer_types"]),      # second blocks: no shortcut conv
]
# fixtures of the reference's own classes (tools/gen_golden_kmax_pixel_decoder.py), one frame each
FIXTURES = [Case("g26_kpix_A", 2611, (65, 97), 1, (256, 512, 1024, 2048), **_SHIPPED),
            Case("g26_kpix_B", 2612, (64, 96), 1, (256, 512, 1024, 2048), **_SHIPPED)]
FIXTURE_FULL = 30000       # a fixture holds an output of up to this many elements in full, of a larger one sums and its last row
BY_NAME = {c.name: c for c in CASES}

# Stage cases: (h, w, base filter, N) of one axial block / axis pass
AXIAL_STAGE_CASES = [(25, 43, 512, 2), (49, 85, 256, 1), (72, 2, 512, 1), (128, 3, 256, 1), (3, 128, 256, 1), (1, 1, 256, 2), (17, 33, 128, 2),
                     (16, 64, 256, 1)]
# (h, w, base filter, N) of one bottleneck block
BOTTLENECK_STAGE_CASES = [(97, 169, 128, 1), (193, 337, 64, 1), (1, 1, 64, 2), (2, 3, 128, 2), (17, 33, 64, 1)]
# ((hl, wl), (h, w), low channels / 4, high channels, out channels, N): the last two lack the high / the low convolution
FUSE_STAGE_CASES = [((25, 43), (49, 85), 512, 1024, 256, 1), ((4, 6), (8, 12), 256, 512, 128, 2), ((1, 1), (2, 2), 128, 256, 64, 2),
                    ((3, 5), (5, 9), 128, 64, 64, 1), ((4, 5), (8, 10), 32, 256, 128, 1)]


def query_shapes(spatial):
    return [(spatial[0] // s + spatial[0] % 2, spatial[1] // s + spatial[1] % 2) for s in STRIDES]


def input_shape(case):
    """what KMaXPixelDecoder takes: name -> an object with channels and stride"""
    return {f"res{2 + i}": types.SimpleNamespace(channels=c, stride=4 * 2 ** i) for i, c in enumerate(case.in_channels)}


def _bn(s, p, c):
    s[p + "weight"], s[p + "bias"], s[p + "running_mean"], s[p + "running_var"], s[p + "num_batches_tracked"] = (c,), (c,), (c,), (c,), ()


def _convbn(s, p, cout, cin, k=(1, 1), norm=True):
    s[p + "conv.weight"] = (cout, cin) + tuple(k)
    if norm:
        _bn(s, p + "norm.", cout)


def _axis(s, p, in_planes, b):
    _convbn(s, p + "qkv_transform.", 4 * b, in_planes, (1,), norm=False)
    s[p + "_query_rpe._embeddings.weight"] = (2 * MAX_SPAN - 1, b // 8)
    s[p + "_key_rpe._embeddings.weight"] = (2 * MAX_SPAN - 1, b // 8)
    s[p + "_value_rpe._embeddings.weight"] = (2 * MAX_SPAN - 1, b // 4)
    _bn(s, p + "_batch_norm_qkv.", 4 * b)
    _bn(s, p + "_batch_norm_similarity.", 24)
    _bn(s, p + "_batch_norm_retrieved_output.", 4 * b)


def block_shapes(s, p, cin, b, axial):
    mid = 2 * b if axial else b
    _convbn(s, p + "_conv1_bn_act.", mid, cin)
    if axial:
        _axis(s, p + "_attention._height_axis.", mid, b)
        _axis(s, p + "_attention._width_axis.", mid, b)
    else:
        _convbn(s, p + "_conv2_bn_act.", b, b, (3, 3))
    _convbn(s, p + "_conv3_bn.", 4 * b, mid)
    if cin != 4 * b:
        _convbn(s, p + "_shortcut.", 4 * b, cin)


def param_shapes(case):
    """state-dict keys of the decoder (the reference's own names, in its registration order) -> shapes"""
    s = OrderedDict()
    cin = case.in_channels[::-1]          # res5 first
    for i in range(4):
        s[f"_in_norms.{i}.weight"], s[f"_in_norms.{i}.bias"] = (cin[i],), (cin[i],)
    for i in range(4):
        b = case.dec_channels[i]
        for j in range(case.dec_layers[i]):
            block_shapes(s, f"_stages.{i}._blocks.{j}.", 4 * b if j else (cin[0] if i == 0 else b), b, case.layer_types[i] == "axial")
    for i in range(1, 4):
        low, high, b = 4 * case.dec_channels[i - 1], cin[i], case.dec_channels[i]
        if low != b:
            _convbn(s, f"_resized_fuses.{i - 1}._conv_bn_low.", b, low)
        if high != b:
            _convbn(s, f"_resized_fuses.{i - 1}._conv_bn_high.", b, high)
    return s


def draw(shapes, seed):
    """fp32 values.  Convolutions N(0, 1/fan_in) (unit gain: activations keep their scale), position tables N(0, 0.05), LayerNorm and
    BatchNorm gains 1 + U(-0.1, 0.1) -- not the reference's zero gain of `_conv3_bn.norm`, which would switch every block off -- except:
    the similarity norm's gains 0.3 + U(-0.1, 0.1) and `_conv3_bn.norm`'s 0.5 + U(-0.1, 0.1), which keep the softmax soft and the residual
    chain of six axial blocks at O(1-10); biases and running means U(-0.1, 0.1), running variances U(0.5, 1.5)."""
    g = torch.Generator().manual_seed(seed)
    out = OrderedDict()
    u = lambda shp: torch.rand(shp, generator=g) * 2 - 1
    for k, shp in shapes.items():
        if k.endswith("num_batches_tracked"):
            out[k] = torch.tensor(0, dtype=torch.long)
            continue
        if k.endswith("conv.weight"):
            v = torch.randn(shp, generator=g) / math.sqrt(math.prod(shp[1:]))
        elif k.endswith("_embeddings.weight"):
            v = 0.05 * torch.randn(shp, generator=g)
        elif k.endswith("running_var"):
            v = 1.0 + 0.5 * u(shp)
        elif k.endswith("_batch_norm_similarity.weight"):
            v = 0.3 + 0.1 * u(shp)
        elif k.endswith("_conv3_bn.norm.weight"):
            v = 0.5 + 0.1 * u(shp)
        elif k.endswith("weight"):
            v = 1.0 + 0.1 * u(shp)
        else:
            v = 0.1 * u(shp)
        out[k] = v.float()
    return out


def make_params(case, seed=None):
    return draw(param_shapes(case), case.seed if seed is None else seed)


def make_inputs(case, seed=None):
    """features res2 .. res5, [N, C_i, h_i, w_i] fp32 N(0, 1)"""
    g = torch.Generator().manual_seed((case.seed if seed is None else seed) + 1)
    sizes = query_shapes(case.spatial)[::-1]          # res2 first
    return {f"res{2 + i}": torch.randn(case.N, c, *sizes[i], generator=g) for i, c in enumerate(case.in_channels)}


def _rpe(table, L):
    """RelativePositionalEncoding.forward: [L, L, d] by gather, entry (l, m) = table[m - l + MAX_SPAN - 1]"""
    idx = torch.arange(L)[None, :] - torch.arange(L)[:, None] + MAX_SPAN - 1
    return table[idx.reshape(-1)].reshape(L, L, table.shape[1])


class Restatement:
    """The decoder's eval forward in `dtype`, from a state dict under the reference's names."""

    def __init__(self, params, dtype):
        self.p = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in params.items()}
        self.dtype = dtype

    def softmax(self, sim):
        """the axial attention's softmax over the keys: a method, so that a test can record its scores or state it wrongly"""
        return F.softmax(sim, dim=-1)

    def bn(self, x, p):
        q = self.p
        return F.batch_norm(x, q[p + "running_mean"], q[p + "running_var"], q[p + "weight"], q[p + "bias"], False, 0.01, EPS)

    def convbn(self, x, p, act=False, **kw):
        w = self.p[p + "conv.weight"]
        x = (F.conv1d if w.dim() == 3 else F.conv2d)(x, w, None, **kw)
        if p + "norm.weight" in self.p:
            x = self.bn(x, p + "norm.")
        return F.gelu(x) if act else x

    def layer_norm(self, x, i):
        x = x.to(self.dtype)
        u = x.mean(1, keepdim=True)
        s = (x - u).pow(2).mean(1, keepdim=True)
        x = (x - u) / torch.sqrt(s + 1e-6)
        return self.p[f"_in_norms.{i}.weight"][:, None, None] * x + self.p[f"_in_norms.{i}.bias"][:, None, None]

    def qkv(self, x, p):
        """x [N, C, L] -> the normalised qkv [N, 4b, L]"""
        return self.bn(self.convbn(x, p + "qkv_transform."), p + "_batch_norm_qkv.")

    def attend(self, qkv, p):
        """AxialAttention.forward behind its qkv norm: qkv [N, 4b, L] -> [N, 2b, L]"""
        N, C4, L = qkv.shape
        kd, vd, H = C4 // 4, C4 // 2, 8
        q, k, v = torch.split(qkv, [kd, kd, vd], dim=1)
        q, k, v = q.reshape(N, H, kd // H, L), k.reshape(N, H, kd // H, L), v.reshape(N, H, vd // H, L)
        content = torch.einsum("bhdl,bhdm->bhlm", q, k)
        q_sim = torch.einsum("bhdl,lmd->bhlm", q, _rpe(self.p[p + "_query_rpe._embeddings.weight"], L))
        k_sim = torch.einsum("bhdm,lmd->bhlm", k, _rpe(self.p[p + "_key_rpe._embeddings.weight"], L))
        sim = torch.cat([content, q_sim, k_sim], dim=1)
        sim = self.bn(sim, p + "_batch_norm_similarity.").reshape(N, 3, H, L, L).sum(dim=1)
        w = self.softmax(sim)
        got = torch.einsum("bhlm,bhdm->bhdl", w, v)
        got_rpe = torch.einsum("bhlm,lmd->bhdl", w, _rpe(self.p[p + "_value_rpe._embeddings.weight"], L))
        out = torch.cat([got, got_rpe], dim=1).reshape(N, 2 * vd, L)
        return self.bn(out, p + "_batch_norm_retrieved_output.").reshape(N, 2, vd, L).sum(1)

    def attention2d(self, x, p, record=None):
        N, C, H, W = x.shape
        x = x.permute(0, 3, 1, 2).contiguous().reshape(N * W, C, H)
        qh = self.qkv(x, p + "_height_axis.")
        x = self.attend(qh, p + "_height_axis.")
        vd = x.shape[1]
        x = x.reshape(N, W, vd, H).permute(0, 3, 2, 1).contiguous().reshape(N * H, vd, W)
        qw = self.qkv(x, p + "_width_axis.")
        y = self.attend(qw, p + "_width_axis.")
        if record is not None:      # channels-last [N, h, w, .]: what the axis-pass entry reads and writes
            record.update(qkv_h=qh.reshape(N, W, -1, H).permute(0, 3, 1, 2), out_h=x.reshape(N, H, vd, W).permute(0, 1, 3, 2),
                          qkv_w=qw.reshape(N, H, -1, W).permute(0, 1, 3, 2), out_w=y.reshape(N, H, vd, W).permute(0, 1, 3, 2))
        return y.reshape(N, H, vd, W).permute(0, 2, 1, 3).contiguous()

    def block(self, x, p, record=None):
        """SingleBlock.forward"""
        x = F.gelu(x.to(self.dtype))
        shortcut = self.convbn(x, p + "_shortcut.") if p + "_shortcut.conv.weight" in self.p else x
        x = self.convbn(x, p + "_conv1_bn_act.", True)
        if p + "_conv2_bn_act.conv.weight" in self.p:
            x = self.convbn(x, p + "_conv2_bn_act.", True, padding=1)
        else:
            x = F.gelu(self.attention2d(x, p + "_attention.", record))
        return self.convbn(x, p + "_conv3_bn.") + shortcut

    def fuse(self, low, high_feature, index):
        """ResizedFuse.forward on a stage's raw output and LN(the backbone feature)"""
        p = f"_resized_fuses.{index}."
        low, high = low.to(self.dtype), self.layer_norm(high_feature, index + 1)
        ac = low.shape[-1] % 2 == 1
        if p + "_conv_bn_low.conv.weight" in self.p:
            low = self.convbn(F.gelu(low), p + "_conv_bn_low.")
        low = F.interpolate(low, size=high.shape[2:], mode="bilinear", align_corners=ac)
        if p + "_conv_bn_high.conv.weight" in self.p:
            high = self.convbn(F.gelu(high), p + "_conv_bn_high.")
        return low + high

    def run(self, features, dec_layers):
        """free run on features res2 .. res5 -> (per-step records: block inputs / outputs and fuse inputs / outputs, the four stage outputs)"""
        feats = [features[k] for k in sorted(features, reverse=True)]
        x, out, rec = self.layer_norm(feats[0], 0), [], []
        for i in range(4):
            if i:
                y = self.fuse(x, feats[i], i - 1)
                rec.append(dict(kind="fuse", index=i - 1, low=x, high=feats[i], out=y))
                x = y
            for j in range(dec_layers[i]):
                y = self.block(x, f"_stages.{i}._blocks.{j}.")
                rec.append(dict(kind="block", stage=i, index=j, x=x, out=y))
                x = y
            out.append(x)
        return rec, out


OUTPUTS = ("stage0", "stage1", "stage2", "panoptic")
_CACHE = {}


def err(a, b):
    return float((a.double().cpu() - b.double().cpu()).abs().max())


def study(case, seed=None):
    """Everything the tests of one whole-decoder case share, computed once and left unchanged: the float64 and float32 free runs, the
    float32 restatement teacher-forced on the float64 chain's step inputs, and the tolerances 8 x (float32 restatement - float64)."""
    key = (case.name, seed)
    if key in _CACHE:
        return _CACHE[key]
    with torch.no_grad():
        params, feats = make_params(case, seed), make_inputs(case, seed)
        r64, r32 = Restatement(params, torch.float64), Restatement(params, torch.float32)
        rec, out64 = r64.run(feats, case.dec_layers)
        _, out32 = r32.run(feats, case.dec_layers)
        for y in rec:       # teacher-forced float32 step on the float64 inputs
            if y["kind"] == "fuse":
                tf = r32.fuse(y["low"].float(), y["high"], y["index"])
            else:
                tf = r32.block(y["x"].float(), f"_stages.{y['stage']}._blocks.{y['index']}.")
            y["tol"] = 8 * err(tf, y["out"])
        st = dict(case=case, params=params, feats=feats, steps=rec, out=dict(zip(OUTPUTS, out64)), out32=dict(zip(OUTPUTS, out32)),
                  tol={k: 8 * err(a, b) for k, a, b in zip(OUTPUTS, out32, out64)})
    _CACHE[key] = st
    return st


# ---- stage cases: one block (or fuse) of a small decoder whose other stages are as light as the bounds allow -------------------------------------
def axial_stage_case(h, w, b, N):
    """a decoder whose stage 0 is one axial block of base filter b on 32 input channels"""
    return Case(f"ax_{h}x{w}_{b}", 2700 + h * 7 + w * 3 + b, None, N, (16, 16, 16, 32), (1, 1, 1, 1), (b, 32, 32, 32),
                ("axial", "bottleneck", "bottleneck", "bottleneck"))


def bottleneck_stage_case(h, w, b, N):
    """a decoder whose stage 3 is one bottleneck block of base filter b (its input: b channels, so it has a shortcut conv)"""
    return Case(f"bn_{h}x{w}_{b}", 2800 + h * 7 + w * 3 + b, None, N, (16, 16, 16, 16), (1, 1, 1, 1), (32, 32, 32, b),
                ("bottleneck", "bottleneck", "bottleneck", "bottleneck"))


def fuse_stage_case(lo, hi, b_prev, high_c, b, N):
    """a decoder whose fuse 0 takes 4 b_prev low channels and high_c high channels to b (stage 0 axial where b_prev is an axial base filter)"""
    return Case(f"fu_{lo[0]}x{lo[1]}_{b_prev}_{high_c}_{b}", 2900 + lo[0] * 7 + lo[1] * 3 + b, None, N, (16, 16, high_c, 16), (1, 1, 1, 1),
                (b_prev, b, 32, 32), ("axial" if b_prev >= 128 else "bottleneck",) + ("bottleneck",) * 3)


def stage_study(kind, spec):
    """(case, params, inputs, float64 record, tolerances) of one stage case, computed once"""
    key = (kind, spec)
    if key in _CACHE:
        return _CACHE[key]
    with torch.no_grad():
        if kind == "axial":
            h, w, b, N = spec
            case = axial_stage_case(*spec)
        elif kind == "bottleneck":
            h, w, b, N = spec
            case = bottleneck_stage_case(*spec)
        else:
            case = fuse_stage_case(*spec)
        params = make_params(case)
        g = torch.Generator().manual_seed(case.seed + 1)
        r64, r32 = Restatement(params, torch.float64), Restatement(params, torch.float32)
        st = dict(case=case, params=params)
        if kind == "fuse":
            lo, hi, b_prev, high_c, b, N = spec
            low, high = 3 * torch.randn(N, 4 * b_prev, *lo, generator=g), torch.randn(N, high_c, *hi, generator=g)
            out = r64.fuse(low, high, 0)
            st.update(low=low, high=high, out=out, tol=8 * err(r32.fuse(low, high, 0), out))
        else:
            stage = 0 if kind == "axial" else 3
            cin = 32 if kind == "axial" else b
            x = 2 * torch.randn(N, cin, h, w, generator=g)
            p = f"_stages.{stage}._blocks.0."
            rec64, rec32 = {}, {}
            out = r64.block(x, p, rec64)
            st.update(x=x, stage=stage, out=out, tol=8 * err(r32.block(x, p, rec32), out), rec=rec64)
            if kind == "axial":      # the axis passes, teacher-forced on the float64 qkv rows
                a = p + "_attention."
                for ax, L in (("h", h), ("w", w)):
                    q64 = rec64["qkv_" + ax]                    # [N, h, w, 4b]
                    seq = q64.permute(0, 2, 3, 1) if ax == "h" else q64.permute(0, 1, 3, 2)       # [N, other, 4b, L]
                    got = r32.attend(seq.reshape(-1, seq.shape[2], L).float(), a + ("_height_axis." if ax == "h" else "_width_axis."))
                    got = got.reshape(N, -1, got.shape[1], L)
                    got = got.permute(0, 3, 1, 2) if ax == "h" else got.permute(0, 1, 3, 2)
                    st["tol_" + ax] = 8 * err(got, rec64["out_" + ax])
    _CACHE[key] = st
    return st
