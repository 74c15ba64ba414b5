"""Cases and restatement of the ConvNeXt / ConvNeXtV2 backbone (axial_vs_amd.ConvNeXtBackbone / ConvNeXtV2Backbone).

`Restatement` states the eval forward of both networks once, in the reference's op order (MaXTron_Video-kMaX/kmax_deeplab/modeling/
backbone/convnext.py:15-151, convnextv2.py:15-151): F.pad in front of each patchify convolution (so in front of the downsample layers'
LayerNorm), the channels-first LayerNorm as the reference writes it, F.layer_norm for the channels-last one, torch.norm for GRN.  It
runs in float64 (the yardstick) or float32, whose own error against float64 sizes every bound of the tests: 8 x that error per compared
tensor, this project's standing factor (9 x against fixtures of the reference's own fp32 run).  The reference itself cannot run in
float64: its LayerNorm casts to float.

No hard decision is taken anywhere in these networks, so no case is screened.

`wrong=` makes the restatement wrong on purpose in one of the three ways a kernel of this path can be (tests/test_convnext_cpu.py checks
that each moves the float64 result by far more than the bound, i.e. that the cases can tell): "pad_zero" -- a padded pixel of a
downsample layer as zeros BEHIND the LayerNorm instead of its bias; "halo" -- the depthwise convolution's border replicated instead of
zero; "grn_shared" -- GRN statistics over all frames at once.  A fourth is what an off-by-one in a GEMM's step count does: "k_short" --
the contraction of `pwconv2` and of the downsample convolutions without its last 32 inputs (one k-step of the device's GEMM, in the order
the device contracts in: the hidden units as they stand, the 2 x 2 patch as (ky, kx, c)).
"""
from collections import OrderedDict, namedtuple

import torch
import torch.nn.functional as F

Net = namedtuple("Net", "name seed size N dims depths v2 gamma")
_SMALL = dict(dims=(16, 32, 64, 128), depths=(1, 1, 3, 1))
_DEEP = dict(dims=(16, 32, 48, 64), depths=(3, 3, 27, 3))
NETS = [Net(f"{n}_{'v2' if v2 else 'v1'}", seed + v2, size, N, **kw, v2=bool(v2), gamma=True)
        for n, seed, size, N, kw in (("A", 2701, (65, 97), 2, _SMALL), ("B", 2703, (64, 96), 1, _SMALL), ("C", 2705, (33, 161), 3, _SMALL),
                                     ("deep", 2707, (65, 97), 1, _DEEP)) for v2 in (0, 1)]
LARGE = dict(dims=(192, 384, 768, 1536), depths=(3, 3, 27, 3))
# ConvNeXt-L's widths on a small image (maps 9 x 13, 5 x 7, 3 x 4, 2 x 2): four blocks that contract over 3072 and two over 6144, back to
# back.  Not in NETS: the tests that walk NETS (bit equality, repacking) need no 0.25 GB of parameters
LARGE_NETS = [Net(f"L_{'v2' if v2 else 'v1'}", 2715 + v2, (33, 49), 2, LARGE["dims"], (1, 1, 4, 2), v2=bool(v2), gamma=True) for v2 in (0, 1)]
BY_NAME = {c.name: c for c in NETS + LARGE_NETS}
SHALLOW = [c.name for c in NETS if not c.name.startswith("deep")]
# fixtures of the reference's own classes (tools/gen_golden_convnext.py)
FIXTURES = [Net("g27_cnx_v1", 2711, (65, 97), 1, **_SMALL, v2=False, gamma=True), Net("g27_cnx_v2", 2712, (65, 97), 1, **_SMALL, v2=True, gamma=True)]
OUTPUTS = ("stem", "res2", "res3", "res4", "res5")

# the depthwise kernel's tiles (csrc/axvs_convnext.h): TH x 16 output pixels, 64 channels per pass; the tallest TH of 8, 4, 2 that gives
# N * ceil(h / TH) * ceil(w / 16) >= 512 workgroups is taken, else 2
TILES = ((8, 16), (4, 16), (2, 16))
# (h, w, C, N) of one depthwise 7x7 + LayerNorm: maps smaller than the halo, the real res5 map (every channel chunk); then the tile size
# + 1 in each direction: the 2-row tile (a part chunk of channels behind a whole one), and the maps at which the 8-row tile (16 x 34 =
# 544 workgroups) and the 4-row tile (8 x 34 = 272 of 8 rows, 16 x 34 of 4) are taken, each one row and one column past whole tiles
DWLN_CASES = [(1, 1, 16, 2), (3, 5, 32, 1), (6, 7, 48, 1), (7, 7, 192, 1), (9, 13, 16, 2), (17, 33, 64, 1), (8, 130, 192, 1), (25, 43, 1536, 1),
              (TILES[2][0] + 1, TILES[2][1] + 1, 80, 1), (15 * TILES[0][0] + 1, 33 * 16 + 1, 16, 1), (15 * TILES[1][0] + 1, 33 * 16 + 1, 16, 1)]
# image sizes of the stem: all four residues of (H + 3) mod 4
STEM_CASES = [(1, 1), (2, 3), (5, 9), (32, 48), (33, 49), (34, 50), (35, 51)]
# (h, w, C) of one downsample layer (C -> 2 C): odd sizes have the padded row / column
# the last one is ConvNeXt-L's deepest downsample layer: a contraction over 4 C = 3072 into 1536 outputs
DOWN_CASES = [(h, w, C) for (h, w) in ((1, 1), (2, 2), (3, 4), (9, 13)) for C in (16, 192)] + [(9, 13, 768)]
# (h, w, N, kind) of one whole block at C = 48: v1, v2, and v1 without gamma
BLOCK_CASES = [(h, w, N, kind) for (h, w, N) in ((1, 1, 1), (5, 7, 2), (17, 25, 3)) for kind in ("v1", "v2")] + [(5, 7, 2, "v1_nogamma")]
# (h, w, N, kind, C) of whole blocks at the widths of ConvNeXt-L's last two stages: `pwconv2` contracts over 4 C = 3072 and 6144, the
# deepest contractions of the library.  Without gamma nothing scales the pwconv2 error down in front of the residual; v2 runs pwconv2 once
# per frame on GRN-scaled weights
DEEP_BLOCK_CASES = [(9, 13, N, kind, C) for C in (768, 1536) for N, kind in ((1, "v1_nogamma"), (2, "v2"))]


def map_sizes(H, W):
    h, w = (H + 3) // 4, (W + 3) // 4
    out = []
    for _ in range(4):
        out.append((h, w))
        h, w = (h + 1) // 2, (w + 1) // 2
    return out


def param_shapes(dims, depths, v2, gamma=True):
    """state-dict keys of the network (the reference's own names) -> shapes"""
    s = OrderedDict()
    s["downsample_layers.0.0.weight"], s["downsample_layers.0.0.bias"] = (dims[0], 3, 4, 4), (dims[0],)
    s["downsample_layers.0.1.weight"], s["downsample_layers.0.1.bias"] = (dims[0],), (dims[0],)
    for i in range(1, 4):
        s[f"downsample_layers.{i}.0.weight"], s[f"downsample_layers.{i}.0.bias"] = (dims[i - 1],), (dims[i - 1],)
        s[f"downsample_layers.{i}.1.weight"], s[f"downsample_layers.{i}.1.bias"] = (dims[i], dims[i - 1], 2, 2), (dims[i],)
    for i in range(4):
        d = dims[i]
        for j in range(depths[i]):
            p = f"stages.{i}.{j}."
            if not v2 and gamma:
                s[p + "gamma"] = (d,)
            s[p + "dwconv.weight"], s[p + "dwconv.bias"] = (d, 1, 7, 7), (d,)
            s[p + "norm.weight"], s[p + "norm.bias"] = (d,), (d,)
            s[p + "pwconv1.weight"], s[p + "pwconv1.bias"] = (4 * d, d), (4 * d,)
            if v2:
                s[p + "grn.gamma"], s[p + "grn.beta"] = (1, 1, 1, 4 * d), (1, 1, 1, 4 * d)
            s[p + "pwconv2.weight"], s[p + "pwconv2.bias"] = (d, 4 * d), (d,)
    return s


def draw(shapes, seed):
    """fp32 values, drawn so that every part matters.  Convolutions and Linear layers N(0, 1/fan_in); LayerNorm weights 1 + U(-0.1, 0.1);
    every bias U(-0.1, 0.1) (a LayerNorm's non-zero bias is what a padded pixel must carry); the layer scale `gamma` U(0.1, 0.6), not the
    1e-6 initial value that would switch every block off; `grn.gamma` 0.3 + U(-0.2, 0.2) and `grn.beta` U(-0.1, 0.1), not their initial
    zeros, which would hide a wrong GRN."""
    g = torch.Generator().manual_seed(seed)
    out = OrderedDict()
    u = lambda shp: torch.rand(shp, generator=g) * 2 - 1
    for k, shp in shapes.items():
        if k.endswith("grn.gamma"):
            out[k] = 0.3 + 0.2 * u(shp)
        elif k.endswith(".gamma"):
            out[k] = 0.35 + 0.25 * u(shp)
        elif len(shp) >= 2 and not k.endswith("grn.beta"):
            fan_in = 1
            for n in shp[1:]:
                fan_in *= n
            out[k] = torch.randn(shp, generator=g) / fan_in ** 0.5
        elif k.endswith("weight"):
            out[k] = 1 + 0.1 * u(shp)
        else:
            out[k] = 0.1 * u(shp)
    return out


def net_params(case):
    return draw(param_shapes(case.dims, case.depths, case.v2, case.gamma), case.seed)


def net_input(case):
    g = torch.Generator().manual_seed(case.seed + 50)
    return torch.randn(case.N, 3, *case.size, generator=g)


class Restatement:
    """maps are NCHW between the steps, as in the reference"""

    def __init__(self, params, dtype, wrong=None):
        self.p = {k: v.to(dtype) for k, v in params.items()}
        self.dtype, self.wrong = dtype, wrong
        self.v2 = any(k.endswith("grn.gamma") for k in params)

    def ln_first(self, x, p):
        w, b = self.p[p + "weight"], self.p[p + "bias"]
        u = x.mean(1, keepdim=True)
        s = (x - u).pow(2).mean(1, keepdim=True)
        x = (x - u) / torch.sqrt(s + 1e-6)
        return w[:, None, None] * x + b[:, None, None]

    def stem(self, x):
        x = F.pad(x, (1, 2, 1, 2, 0, 0, 0, 0), "constant", 0)
        x = F.conv2d(x, self.p["downsample_layers.0.0.weight"], self.p["downsample_layers.0.0.bias"], stride=4)
        return self.ln_first(x, "downsample_layers.0.1.")

    def down(self, x, i):
        p = f"downsample_layers.{i}."
        if self.wrong == "pad_zero":
            x = F.pad(self.ln_first(x, p + "0."), (0, 1, 0, 1, 0, 0, 0, 0), "constant", 0)
        else:
            x = self.ln_first(F.pad(x, (0, 1, 0, 1, 0, 0, 0, 0), "constant", 0), p + "0.")
        w = self.p[p + "1.weight"]
        if self.wrong == "k_short":
            w = w.clone()
            w[:, -32:, 1, 1] = 0
        return F.conv2d(x, w, self.p[p + "1.bias"], stride=2)

    def dwln(self, x, p):
        """-> channels-last [N, h, w, C]"""
        C = x.shape[1]
        if self.wrong == "halo":
            x = F.conv2d(F.pad(x, (3, 3, 3, 3), "replicate"), self.p[p + "dwconv.weight"], self.p[p + "dwconv.bias"], groups=C)
        else:
            x = F.conv2d(x, self.p[p + "dwconv.weight"], self.p[p + "dwconv.bias"], padding=3, groups=C)
        x = x.permute(0, 2, 3, 1)
        return F.layer_norm(x, (C,), self.p[p + "norm.weight"], self.p[p + "norm.bias"], 1e-6)

    def grn(self, x, p):
        Gx = torch.norm(x, p=2, dim=(0, 1, 2) if self.wrong == "grn_shared" else (1, 2), keepdim=True)
        Nx = Gx / (Gx.mean(dim=-1, keepdim=True) + 1e-6)
        return self.p[p + "gamma"] * (x * Nx) + self.p[p + "beta"] + x

    def block(self, x, p):
        inp = x
        x = self.dwln(x, p)
        x = F.linear(x, self.p[p + "pwconv1.weight"], self.p[p + "pwconv1.bias"])
        x = F.gelu(x)
        if self.v2:
            x = self.grn(x, p + "grn.")
        if self.wrong == "k_short":
            x = F.linear(x[..., :-32], self.p[p + "pwconv2.weight"][:, :-32], self.p[p + "pwconv2.bias"])
        else:
            x = F.linear(x, self.p[p + "pwconv2.weight"], self.p[p + "pwconv2.bias"])
        if p + "gamma" in self.p:
            x = self.p[p + "gamma"] * x
        return inp + x.permute(0, 3, 1, 2)

    def forward(self, x, depths, steps=None):
        """-> {stem, res2 .. res5}; steps (a list): every step's (kind, index, input, output) is appended"""
        outs = {}
        x = x.to(self.dtype)
        for i in range(4):
            y = self.stem(x) if i == 0 else self.down(x, i)
            if steps is not None:
                steps.append(("down", i, x, y))
            x = y
            if i == 0:
                outs["stem"] = x
            for j in range(depths[i]):
                y = self.block(x, f"stages.{i}.{j}.")
                if steps is not None:
                    steps.append(("block", (i, j), x, y))
                x = y
            outs[f"res{i + 2}"] = x
        return outs


def cpu_probe():
    """A fingerprint of this CPU's float32 arithmetic in the op kinds and sizes of the fixtures' networks (seeded data, nothing of the
    restatement or of the reference in it).  torch's CPU kernels differ between processors (vector width, blocking), so float32
    results are equal bit for bit only between machines whose probes are equal: the fixtures record their generator's probe."""
    import hashlib
    g = torch.Generator().manual_seed(2799)
    r = lambda *s: torch.randn(*s, generator=g)
    x = r(1, 3, 65, 97)
    ts = [F.conv2d(F.pad(x, (1, 2, 1, 2)), r(16, 3, 4, 4) / 7, r(16), stride=4)]
    for C, h, w in ((16, 17, 25), (32, 9, 13), (64, 5, 7), (128, 3, 4)):
        y = r(1, C, h, w)
        d = F.conv2d(y, r(C, 1, 7, 7) / 7, r(C), padding=3, groups=C).permute(0, 2, 3, 1)
        n = F.layer_norm(d, (C,), r(C), r(C), 1e-6)
        hid = F.gelu(F.linear(n, r(4 * C, C) / C ** 0.5, r(4 * C)))
        ts += [d, n, hid, torch.norm(hid, p=2, dim=(1, 2), keepdim=True), F.linear(hid, r(C, 4 * C) / (4 * C) ** 0.5, r(C)), y.mean(1, keepdim=True),
               (y - y.mean(1, keepdim=True)).pow(2).mean(1, keepdim=True), F.conv2d(F.pad(y, (0, 1, 0, 1)), r(2 * C, C, 2, 2) / (4 * C) ** 0.5, r(2 * C), stride=2)]
    return hashlib.sha1(b"".join(t.contiguous().numpy().tobytes() for t in ts)).hexdigest()


def err(got, want):
    """max |got - want| in float64"""
    return float((got.detach().double().cpu() - want.double()).abs().max())


def rows(x):
    """NCHW -> channels-last [N, h, w, C], contiguous"""
    return x.permute(0, 2, 3, 1).contiguous()


_STUDY = {}


def _once(key, make):
    if key not in _STUDY:
        with torch.no_grad():
            _STUDY[key] = make()
    return _STUDY[key]


def _teacher(r64, r32, fn, x64):
    """one step on the float64 input and on its float32 rounding: (float32 input, float64 output, the float32 restatement's error)"""
    x32 = x64.float()
    want = fn(r64, x64)
    return x32, want, err(fn(r32, x32), want)


def study(case):
    """params, input, the float64 outputs `want`, the float32 restatement's `tol` = 8 x its error per output, and `steps`: every step
    teacher-forced on the float64 chain ({kind, index, x (float32, NCHW), out (float64, NCHW), tol})"""
    def make():
        params, x = net_params(case), net_input(case)
        r64, r32 = Restatement(params, torch.float64), Restatement(params, torch.float32)
        rec = []
        want = r64.forward(x, case.depths, rec)
        got32 = r32.forward(x, case.depths)
        steps = []
        for kind, index, xin, out in rec:
            if kind == "down":
                fn = (lambda r, t: r.stem(t)) if index == 0 else (lambda r, t, i=index: r.down(t, i))
            else:
                fn = lambda r, t, p=f"stages.{index[0]}.{index[1]}.": r.block(t, p)
            e = err(fn(r32, xin.float()), out)
            steps.append(dict(kind=kind, index=index, x=xin.float(), out=out, tol=8 * e))
        return dict(params=params, x=x, want=want, f32=got32, tol={k: 8 * err(got32[k], want[k]) for k in OUTPUTS}, steps=steps)
    return _once(("net", case.name), make)


def _stage_params(dims, v2, gamma, seed):
    return draw(param_shapes(dims, (1, 1, 1, 1), v2, gamma), seed)


def dwln_study(spec, wrong=None):
    """-> params of a network whose stage 0 has C channels, x [N, h, w, C] float32 (channels-last), out float64 alike, tol"""
    h, w, C, N = spec

    def make():
        params = _stage_params((C, 16, 16, 16), False, True, 2720 + h * 7 + w)
        x = torch.randn(N, C, h, w, generator=torch.Generator().manual_seed(2721 + h + w), dtype=torch.float64)
        fn = lambda r, t: r.dwln(t, "stages.0.0.")
        x32, want, e = _teacher(Restatement(params, torch.float64, wrong), Restatement(params, torch.float32), fn, x)
        return dict(params=params, dims=(C, 16, 16, 16), x=rows(x32), out=want, tol=8 * e)
    return _once(("dwln", spec, wrong), make)


def stem_study(size, wrong=None):
    """image [2, 3, H, W] float32 -> out float64 [2, h, w, 32] (channels-last)"""
    def make():
        dims = (32, 16, 16, 16)
        params = _stage_params(dims, False, True, 2730 + size[0])
        x = torch.randn(2, 3, *size, generator=torch.Generator().manual_seed(2731 + size[1]), dtype=torch.float64)
        x32, want, e = _teacher(Restatement(params, torch.float64, wrong), Restatement(params, torch.float32), lambda r, t: r.stem(t), x)
        return dict(params=params, dims=dims, x=x32, out=rows(want), tol=8 * e)
    return _once(("stem", size, wrong), make)


def down_study(spec, wrong=None):
    """x [2, h, w, C] float32 (channels-last) -> out float64 [2, h2, w2, 2 C] of downsample layer 1"""
    h, w, C = spec

    def make():
        dims = (C, 2 * C, 16, 16)
        params = _stage_params(dims, False, True, 2740 + h + C)
        x = torch.randn(2, C, h, w, generator=torch.Generator().manual_seed(2741 + w), dtype=torch.float64)
        x32, want, e = _teacher(Restatement(params, torch.float64, wrong), Restatement(params, torch.float32), lambda r, t: r.down(t, 1), x)
        return dict(params=params, dims=dims, x=rows(x32), out=rows(want), tol=8 * e)
    return _once(("down", spec, wrong), make)


def block_study(spec, wrong=None, C=48):
    """x [N, h, w, C] float32 (channels-last; frame n scaled by 1 + n, so that the frames' GRN statistics differ) -> out float64 alike"""
    h, w, N, kind = spec

    def make():
        dims = (C, 16, 16, 16)
        params = _stage_params(dims, kind == "v2", kind != "v1_nogamma", 2750 + h + N)
        x = torch.randn(N, C, h, w, generator=torch.Generator().manual_seed(2751 + w), dtype=torch.float64)
        x = x * (1 + torch.arange(N, dtype=torch.float64))[:, None, None, None]
        fn = lambda r, t: r.block(t, "stages.0.0.")
        x32, want, e = _teacher(Restatement(params, torch.float64, wrong), Restatement(params, torch.float32), fn, x)
        return dict(params=params, dims=dims, v2=kind == "v2", gamma=kind != "v1_nogamma", x=rows(x32), out=rows(want), tol=8 * e)
    return _once(("block", spec, wrong, C), make)
