"""Cases and restatement of the ResNet bottleneck backbone (axial_vs_amd.ResNetBackbone).

`Restatement` states the eval forward once, in the reference's op order and unfused (MaXTron_Video-kMaX/kmax_deeplab/modeling/backbone/
resnet.py:103-214, 333-493): F.conv2d, F.batch_norm on the running statistics (eps 1e-3, the reference's get_norm), ReLU, F.max_pool2d,
the sum with the shortcut, ReLU.  It runs in float64 (the yardstick) or float32, whose own error against float64 sizes every bound of
the tests: 8 x that error per compared tensor, this project's standing factor (9 x against fixtures of the reference's own fp32 run).

No hard decision is taken anywhere in the network (a ReLU and a maximum are continuous), so no case is screened.

Parameters are drawn so that every part matters: convolutions N(0, 1/fan_in); BatchNorm weight 1 + 0.3 U(-1, 1), bias 0.2 U, running_mean
0.3 U, running_var 1 + 0.5 U.

`wrong=` makes the restatement wrong on purpose in one of the ways a kernel of this path can be (tests/test_resnet_cpu.py checks that each
moves the float64 result by far more than the bound): "stride_phase" -- a stride-2 3x3 centred on pixel 2y + 1 instead of 2y;
"shortcut_phase" -- the same for a strided 1x1; "dilation_pad" -- a dilated 3x3 whose taps start one pixel, not `dilation` pixels, in front
of the output pixel; "relu_before_add" -- the block's last ReLU in front of the sum with the shortcut; "k_short" -- a block's first 1x1
(its deepest contraction) without its last 32 input channels, one k-step of the device's GEMM, what an off-by-one in a step count does.
"""
from collections import OrderedDict, namedtuple
import ctypes
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-3
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
Net = namedtuple("Net", "name seed size N stem widths outs blocks stride_in_1x1 res5_dilation")
_SMALL = dict(stem=32, widths=(32, 64, 128, 256), outs=(128, 256, 512, 1024), blocks=(1, 1, 2, 1))
_DEEP = dict(stem=32, widths=(32, 64, 128, 256), outs=(128, 256, 512, 1024), blocks=(3, 4, 23, 3))
_FORMS = (("a", False, 1), ("b", True, 2))      # (stride_in_1x1, res5_dilation)
NETS = [Net(f"{n}_{f}", seed + (f == "b"), size, N, **_SMALL, stride_in_1x1=s1, res5_dilation=d5)
        for n, seed, size, N in (("A", 2801, (65, 97), 2), ("B", 2803, (64, 96), 1), ("C", 2805, (33, 161), 3)) for f, s1, d5 in _FORMS]
NETS.append(Net("deep", 2807, (65, 97), 1, **_DEEP, stride_in_1x1=False, res5_dilation=1))
BY_NAME = {c.name: c for c in NETS}
# fixtures of the reference's own classes (tools/gen_golden_resnet.py)
FIXTURES = [Net(f"g28_rn_{f}", 2811 + (f == "b"), (65, 97), 1, **_SMALL, stride_in_1x1=s1, res5_dilation=d5) for f, s1, d5 in _FORMS]
OUTPUTS = ("stem", "res2", "res3", "res4", "res5")

# the 3x3 kernel's tiles (csrc/axvs_resnet.h, RnConv3): TH x 16 OUTPUT pixels, TH = 8 at stride 1 and 4 at stride 2, by 128 output channels
# where C > 64 and that still gives WIDE_WGS workgroups (csrc/axvs_resnet.hip, kRnConv3Wgs), else by 64: four forms
TILES = {1: (8, 16), 2: (4, 16)}
WIDE_WGS = 256


def conv3_is_wide(spec):
    h, w, C, N, stride, d = spec
    th, tw = TILES[stride]
    return C > 64 and N * -(-C // 128) * -(-(-(-h // stride)) // th) * -(-(-(-w // stride)) // tw) >= WIDE_WGS


# (h, w, C, N, stride, dilation) of one 3x3 + BatchNorm + ReLU on an h x w input.  Maps smaller than the halo; both parities for stride 2;
# one OUTPUT pixel past whole tiles in each direction for each of the four tile forms, and at dilation 2 (the 128-channel forms need maps
# of 288 workgroups: 9 x 8 tiles by frames and channel tiles); C = 32 (one chunk), 96 (part of an output-channel tile behind nothing
# whole), 160 (a part tile behind a whole one), 512 (every chunk); the real R-50 maps at the VIPSeg clip size: res5's 25 x 43 x 512 at
# dilation 1 and 2, and res5's first block reading res4's 49 x 85 at stride 2
CONV3_CASES = [(1, 1, 32, 2, 1, 1), (2, 3, 32, 1, 2, 1), (3, 5, 64, 1, 1, 2), (8, 9, 64, 1, 2, 1), (9, 8, 64, 1, 2, 1),
               (2 * TILES[1][0] + 1, 2 * TILES[1][1] + 1, 32, 1, 1, 1), (2 * TILES[1][0] + 1, 2 * TILES[1][1] + 1, 96, 2, 1, 1),
               (2 * TILES[1][0] + 1, 2 * TILES[1][1] + 1, 64, 1, 1, 2), (2 * TILES[1][0] + 1, 2 * TILES[1][1] + 1, 160, 1, 1, 2),
               (2 * (2 * TILES[2][0] + 1) - 1, 2 * (2 * TILES[2][1] + 1) - 1, 64, 1, 2, 1), (2 * (2 * TILES[2][0] + 1), 2 * (2 * TILES[2][1] + 1), 160, 2, 2, 1),
               (8 * TILES[1][0] + 1, 7 * TILES[1][1] + 1, 96, 4, 1, 1), (8 * TILES[1][0] + 1, 7 * TILES[1][1] + 1, 160, 2, 1, 2),
               (2 * (8 * TILES[2][0] + 1), 2 * (7 * TILES[2][1] + 1), 160, 2, 2, 1),
               (25, 43, 512, 1, 1, 1), (25, 43, 512, 1, 1, 2), (49, 85, 512, 1, 2, 1)]
assert [conv3_is_wide(s) for s in CONV3_CASES[11:14]] == [True] * 3 and not any(conv3_is_wide(s) for s in CONV3_CASES[:11] + CONV3_CASES[14:])
# the stem's tile (csrc/axvs_resnet.h): 8 x 7 pooled pixels
STEM_TILE = (8, 7)
# image sizes of the stem: tiny images, all four residues of H mod 4, one pooled pixel past the tile in each direction
STEM_CASES = [(1, 1), (2, 3), (5, 9), (7, 7), (32, 48), (33, 49), (34, 50), (35, 51), (4 * STEM_TILE[0] + 1, 4 * STEM_TILE[1] + 1)]
# (h, w, N, kind) of one whole block
BLOCK_KINDS = ("identity", "proj_s1", "proj_s2", "s2_in_1x1", "dil2")
BLOCK_CASES = [(h, w, N, kind) for (h, w, N) in ((1, 1, 1), (5, 7, 2), (17, 25, 3)) for kind in BLOCK_KINDS] + [(6, 8, 2, "proj_s2"), (6, 8, 2, "s2_in_1x1")]
# the network the step studies cut their blocks from: (stage, block) of each kind
_STEP = dict(stem=32, widths=(32, 32, 64, 32), outs=(64, 96, 128, 160), blocks=(2, 1, 1, 1))
_KIND_AT = {"identity": (0, 1, False, 1), "proj_s1": (0, 0, False, 1), "proj_s2": (1, 0, False, 1), "s2_in_1x1": (2, 0, True, 1), "dil2": (3, 0, False, 2)}
# R-50's own widths, two blocks in res5: the 1x1 convolutions' contractions at their real depths.  res5.0: the projection shortcut
# 1024 -> 2048, conv1 over 1024, conv3 over 512 with the ReLU behind the residual; res5.1: the identity shortcut, conv1 over 2048;
# res4.0: 512 -> 256 -> 1024.  Both forms: "a" strides in the 3x3, "b" strides in the first 1x1 and dilates res5 instead of striding it
R50_WIDTHS = dict(stem=64, widths=(64, 128, 256, 512), outs=(256, 512, 1024, 2048), blocks=(1, 1, 1, 2))
_KIND_AT.update({f"res{i + 2}.{j}_{f}": (i, j, s1, d5) for i, j in ((3, 0), (3, 1), (2, 0)) for f, s1, d5 in _FORMS})
# (h, w, N, kind) of one whole block of R50_WIDTHS: 5 x 7, and 6 x 8 where the block strides
WIDE_BLOCK_CASES = [((6, 8) if j == 0 and not (i == 3 and d5 == 2) else (5, 7)) + (2, f"res{i + 2}.{j}_{f}") for i, j in ((3, 0), (3, 1), (2, 0)) for f, _, d5 in _FORMS]


def strides_of(case):
    return (1, 2, 2, 1 if case.res5_dilation == 2 else 2)


def stage_sizes(case, H, W):
    """the maps the four stages read, then the map res5 leaves"""
    h, w = ((H + 1) // 2 + 1) // 2, ((W + 1) // 2 + 1) // 2
    out = []
    for s in strides_of(case) + (1,):
        out.append((h, w))
        h, w = -(-h // s), -(-w // s)
    return out


def _conv_bn(s, p, cout, cin, k):
    s[p + "weight"] = (cout, cin, k, k)
    for n in ("weight", "bias", "running_mean", "running_var"):
        s[p + "norm." + n] = (cout,)
    s[p + "norm.num_batches_tracked"] = ()


def param_shapes(case):
    """state-dict keys of the network (the reference's own names, in its order) -> shapes"""
    s = OrderedDict()
    _conv_bn(s, "stem.conv1.", case.stem, 3, 7)
    cin = case.stem
    for i in range(4):
        for j in range(case.blocks[i]):
            p = f"res{i + 2}.{j}."
            if cin != case.outs[i]:
                _conv_bn(s, p + "shortcut.", case.outs[i], cin, 1)
            _conv_bn(s, p + "conv1.", case.widths[i], cin, 1)
            _conv_bn(s, p + "conv2.", case.widths[i], case.widths[i], 3)
            _conv_bn(s, p + "conv3.", case.outs[i], case.widths[i], 1)
            cin = case.outs[i]
    return s


def draw(shapes, seed):
    g = torch.Generator().manual_seed(seed)
    out = OrderedDict()
    u = lambda shp: torch.rand(shp, generator=g) * 2 - 1
    for k, shp in shapes.items():
        if k.endswith("num_batches_tracked"):
            out[k] = torch.tensor(0, dtype=torch.long)
        elif len(shp) == 4:
            out[k] = torch.randn(shp, generator=g) / (shp[1] * shp[2] * shp[3]) ** 0.5
        elif k.endswith("norm.weight"):
            out[k] = 1 + 0.3 * u(shp)
        elif k.endswith("norm.bias"):
            out[k] = 0.2 * u(shp)
        elif k.endswith("running_mean"):
            out[k] = 0.3 * u(shp)
        else:
            out[k] = 1 + 0.5 * u(shp)
    return out


def net_params(case):
    return draw(param_shapes(case), case.seed)


def net_input(case):
    g = torch.Generator().manual_seed(case.seed + 50)
    return torch.randn(case.N, 3, *case.size, generator=g)


class Restatement:
    """maps are NCHW between the steps, as in the reference"""

    def __init__(self, params, dtype, stride_in_1x1=False, res5_dilation=1, wrong=None):
        self.p = {k: v.to(dtype) for k, v in params.items() if v.is_floating_point()}
        self.dtype, self.wrong = dtype, wrong
        self.stride_in_1x1, self.res5_dilation = stride_in_1x1, res5_dilation

    def bn(self, x, p):
        return F.batch_norm(x, self.p[p + "running_mean"], self.p[p + "running_var"], self.p[p + "weight"], self.p[p + "bias"], False, 0.0, EPS)

    def stem(self, x):
        x = F.conv2d(x, self.p["stem.conv1.weight"], None, stride=2, padding=3)
        x = F.relu(self.bn(x, "stem.conv1.norm."))
        return F.max_pool2d(x, kernel_size=3, stride=2, padding=1)

    def conv1x1(self, x, p, stride):
        if stride == 2 and self.wrong == "shortcut_phase":
            x = F.pad(x, (0, 1, 0, 1))[:, :, 1::2, 1::2]
            stride = 1
        w = self.p[p + "weight"]
        if self.wrong == "k_short" and p.endswith("conv1."):
            x, w = x[:, :-32], w[:, :-32]
        return self.bn(F.conv2d(x, w, None, stride=stride), p + "norm.")

    def conv3x3(self, x, p, stride, d):
        """conv2 + BatchNorm + ReLU"""
        w = self.p[p + "weight"]
        if d > 1 and self.wrong == "dilation_pad":
            y = F.conv2d(F.pad(x, (1, 2 * d - 1, 1, 2 * d - 1)), w, None, stride=stride, dilation=d)
        elif stride == 2 and self.wrong == "stride_phase":
            y = F.pad(F.conv2d(x, w, None, padding=d, dilation=d), (0, 1, 0, 1))[:, :, 1::2, 1::2]
        else:
            y = F.conv2d(x, w, None, stride=stride, padding=d, dilation=d)
        return F.relu(self.bn(y, p + "norm."))

    def block(self, x, p, stride, d, inner=None):
        """inner (a list): conv2's (input, output) is appended"""
        s1, s3 = (stride, 1) if self.stride_in_1x1 else (1, stride)
        out = F.relu(self.conv1x1(x, p + "conv1.", s1))
        mid = self.conv3x3(out, p + "conv2.", s3, d)
        if inner is not None:
            inner.append((out, mid))
        out = self.conv1x1(mid, p + "conv3.", 1)
        shortcut = self.conv1x1(x, p + "shortcut.", stride) if p + "shortcut.weight" in self.p else x
        if self.wrong == "relu_before_add":
            return F.relu(out) + shortcut
        return F.relu(out + shortcut)

    def geometry(self, i, j):
        """(stride, dilation) of block j of stage i"""
        d = self.res5_dilation if i == 3 else 1
        first = 1 if i == 0 or (i == 3 and d == 2) else 2
        return (first if j == 0 else 1), d

    def forward(self, x, blocks, steps=None):
        """-> {stem, res2 .. res5}; steps (a list): every step's (kind, index, input, output) is appended"""
        outs = {}
        x = x.to(self.dtype)
        y = self.stem(x)
        if steps is not None:
            steps.append(("stem", None, x, y))
        x = outs["stem"] = y
        for i in range(4):
            for j in range(blocks[i]):
                inner = []
                y = self.block(x, f"res{i + 2}.{j}.", *self.geometry(i, j), inner=inner)
                if steps is not None:
                    steps.append(("conv3", (i, j)) + inner[0])
                    steps.append(("block", (i, j), x, y))
                x = y
            outs[f"res{i + 2}"] = x
        return outs


def restatement(case, params, dtype, wrong=None):
    return Restatement(params, dtype, case.stride_in_1x1, case.res5_dilation, wrong)


def cpu_probe():
    """A fingerprint of this CPU's float32 arithmetic in the op kinds and sizes of the fixtures' networks (seeded data, nothing of the
    restatement or of the reference in it).  torch's CPU kernels differ between processors, so float32 results are equal bit for bit only
    between machines whose probes are equal: the fixtures record their generator's probe."""
    import hashlib
    g = torch.Generator().manual_seed(2899)
    r = lambda *s: torch.randn(*s, generator=g)
    x = r(1, 3, 65, 97)
    y = F.conv2d(x, r(32, 3, 7, 7) / 12, None, stride=2, padding=3)
    ts = [y, F.max_pool2d(F.relu(y), 3, 2, 1)]
    for C, h, w in ((32, 17, 25), (64, 9, 13), (128, 5, 7), (256, 3, 4)):
        t = r(1, 2 * C, h, w)
        a = F.conv2d(t, r(C, 2 * C, 1, 1) / (2 * C) ** 0.5)
        ts += [a, F.batch_norm(a, r(C), r(C).abs() + 0.5, r(C), r(C), False, 0.0, EPS), F.conv2d(a, r(C, C, 3, 3) / (9 * C) ** 0.5, None, stride=2, padding=1),
               F.conv2d(a, r(C, C, 3, 3) / (9 * C) ** 0.5, None, padding=2, dilation=2), F.conv2d(t, r(4 * C, 2 * C, 1, 1) / (2 * C) ** 0.5, None, stride=2)]
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


def _step_fn(kind, index, geometry):
    if kind == "stem":
        return lambda r, t: r.stem(t)
    p = f"res{index[0] + 2}.{index[1]}."
    stride, d = geometry
    if kind == "conv3":
        return lambda r, t: r.conv3x3(t, p + "conv2.", 1 if r.stride_in_1x1 else stride, d)
    return lambda r, t: r.block(t, p, stride, d)


def study(case):
    """params, input, the float64 outputs `want`, the float32 restatement's outputs `f32`, `tol` = 8 x its error per output, and `steps`:
    every step teacher-forced on the float64 chain ({kind, index, x (float32, NCHW), out (float64, NCHW), tol})"""
    def make():
        params, x = net_params(case), net_input(case)
        r64, r32 = restatement(case, params, torch.float64), restatement(case, params, torch.float32)
        rec = []
        want = r64.forward(x, case.blocks, rec)
        got32 = r32.forward(x, case.blocks)
        steps = []
        for kind, index, xin, out in rec:
            fn = _step_fn(kind, index, r64.geometry(*index) if index else None)
            steps.append(dict(kind=kind, index=index, x=xin.float(), out=out, tol=8 * err(fn(r32, xin.float()), out)))
        return dict(params=params, x=x, want=want, f32=got32, tol={k: 8 * err(got32[k], want[k]) for k in OUTPUTS}, steps=steps)
    return _once(("net", case.name), make)


def _teacher(r64, r32, fn, x64):
    """one step on the float64 input and on its float32 rounding: (float32 input, float64 output, the float32 restatement's error)"""
    x32 = x64.float()
    want = fn(r64, x64)
    return x32, want, err(fn(r32, x32), want)


def conv3_study(spec, wrong=None):
    """-> the network (`case`) whose block (`stage`, 0) has the 3x3 of `spec`, its params, x [N, h, w, C] float32 (channels-last), out
    float64 alike, tol"""
    h, w, C, N, stride, d = spec

    def make():
        stage = {(1, 1): 0, (2, 1): 1, (1, 2): 3}[(stride, d)]
        widths = [32] * 4
        widths[stage] = C
        case = Net(f"c3_{'x'.join(map(str, spec))}", 2820 + 7 * h + 3 * w + C, None, N, 16, tuple(widths), (32, 48, 64, 80), (1, 1, 1, 1), False, d)
        params = net_params(case)
        x = torch.randn(N, C, h, w, generator=torch.Generator().manual_seed(2821 + h + w), dtype=torch.float64)
        fn = lambda r, t: r.conv3x3(t, f"res{stage + 2}.0.conv2.", stride, d)
        x32, want, e = _teacher(restatement(case, params, torch.float64, wrong), restatement(case, params, torch.float32), fn, x)
        return dict(case=case, stage=stage, params=params, x=rows(x32), out=rows(want), tol=8 * e)
    return _once(("conv3", spec, wrong), make)


def stem_study(size):
    """image [2, 3, H, W] float32 -> out float64 [2, h, w, 32] (channels-last)"""
    def make():
        case = Net(f"stem_{size[0]}x{size[1]}", 2830 + size[0], size, 2, 32, (32,) * 4, (32, 48, 64, 80), (1, 1, 1, 1), False, 1)
        params = net_params(case)
        x = torch.randn(2, 3, *size, generator=torch.Generator().manual_seed(2831 + size[1]), dtype=torch.float64)
        x32, want, e = _teacher(restatement(case, params, torch.float64), restatement(case, params, torch.float32), lambda r, t: r.stem(t), x)
        return dict(case=case, params=params, x=x32, out=rows(want), tol=8 * e)
    return _once(("stem", size), make)


def block_study(spec, wrong=None, net=_STEP):
    """-> the network (`case`, of the widths `net`) and the (`stage`, `index`) of a block of the kind, x [N, h, w, in] float32
    (channels-last), out float64"""
    h, w, N, kind = spec

    def make():
        stage, index, s1, d5 = _KIND_AT[kind]
        case = Net(f"blk_{kind}", 2840 + h + N, None, N, **net, stride_in_1x1=s1, res5_dilation=d5)
        params = net_params(case)
        cin = case.outs[stage] if index else (case.stem if stage == 0 else case.outs[stage - 1])
        x = torch.randn(N, cin, h, w, generator=torch.Generator().manual_seed(2841 + w), dtype=torch.float64)
        r64 = restatement(case, params, torch.float64, wrong)
        fn = lambda r, t: r.block(t, f"res{stage + 2}.{index}.", *r.geometry(stage, index))
        x32, want, e = _teacher(r64, restatement(case, params, torch.float32), fn, x)
        return dict(case=case, stage=stage, index=index, params=params, x=rows(x32), out=rows(want), tol=8 * e)
    return _once(("block", spec, wrong, net["widths"], net["outs"]), make)


# ---- what both test modules share: fixtures, modules, a C configuration ----------------------------------------------------------------------
def load_fixture(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    m = json.loads(bytes(z["meta"]).decode())
    case = Net(m["name"], m["seed"], tuple(m["size"]), m["N"], m["stem"], tuple(m["widths"]), tuple(m["outs"]), tuple(m["blocks"]), m["stride_in_1x1"],
                  m["res5_dilation"])
    return case, m, z


def make_module(case, device=None, **kw):
    import axial_vs_amd as ax
    with torch.device(device) if device else torch.device("cpu"):
        return ax.ResNetBackbone(depth=None, num_blocks=case.blocks, stem_out_channels=case.stem, bottleneck_channels=case.widths, stage_out_channels=case.outs,
                                 stride_in_1x1=case.stride_in_1x1, res5_dilation=case.res5_dilation, **kw)


def rn_cfg(**kw):
    """an AxvsRnCfg of a small valid network on a 33 x 33 image, with the given fields replaced"""
    from axial_vs_amd import _lib
    i4 = ctypes.c_int * 4
    f = dict(N=1, H=33, W=33, in_channels=3, stem_channels=16, width=(32, 32, 64, 64), out_channels=(32, 48, 64, 80), blocks=(1, 1, 1, 1), stride=(1, 2, 2, 2),
             dilation=(1, 1, 1, 1), h=(9, 9, 5, 3), w=(9, 9, 5, 3), stride_in_1x1=0)
    f.update(kw)
    four = ("width", "out_channels", "blocks", "stride", "dilation", "h", "w")
    return _lib.AxvsRnCfg(**{k: (i4(*v) if k in four else v) for k, v in f.items()})
