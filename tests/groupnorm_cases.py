"""Cases and restatements for the 1x1 convolution + GroupNorm projections (axvs_conv1x1_gn_fwd, axvs_conv1x1_gn_train_fwd / _bwd) at
groups whose mean is many standard deviations: tests/test_groupnorm_cpu.py, tests/test_hip_groupnorm.py.

WHY.  A projection of post-ReLU backbone maps has groups with |mean| / std = r of tens to hundreds.  A variance formed as
E[y^2] - mean^2 from fp32 sums loses r^2 ulps there, a centred one (torch's group_norm) only r.  Every group of a case therefore
belongs to an OFFSET CLASS, its target r: group g of sample 0 has class CLASSES[g % 6] with sign (-1)^(g // 6), sample 1 the same
list reversed (statistics swapped or shared between samples fail), and one group is DEAD: y is constant there and the reference
returns beta exactly.  Errors are taken per class (class_err), never as one norm over the tensor.

FAMILY "exact": the convolution is exact on every GEMM path (16-bit pieces, split-K partials, the NCHW loader), so the statistics and
the apply are the only roundings, and the float64 y is the truth.
    x      integers in [-64, 64] / 64 (7 bits: exact in bf16 and f16); input channels 0 and 1 hold the sample index n (0. or 1.)
    W[o]   +-1 at four distinct input channels >= 2 chosen from o, zero elsewhere; W[o][0], W[o][1] = the sample switch (below)
    bias   per group: (signed class of sample 0) x std(z) - mean(z), z = W x + (o % cg) / 8 of sample 0, rounded to 2^-10; + (o % cg) / 8
    W[o][0:2]  per group: what moves sample 1 from sample 0's offset to its own (the reversed list), in two pieces of 8 significant
           bits (each exact in bf16): a bias is shared by the samples, so the second sample's offset has to come through the convolution
    y      a multiple of 2^-10 below 1024 (20 bits): exact in fp32, and so is every partial sum of the convolution
    gamma = 1 + (o % 5) / 8, beta = (o % 3) / 4 - 0.25
    dead group: W rows zero (the switch too), bias DEAD_VALUE on all its channels: y is that constant in both samples
FAMILY "drawn": the mean goes through the GEMM.  Even input channels are x = relu(randn + 0.5) as on a backbone; the odd ones are
quiet, relu(0.5 + randn / 1024), and lit in one sample only (c % 4 == 1: sample 0, c % 4 == 3: sample 1; zero in the other).
W = randn / sqrt(Cin) + k[n, g] / Cin on the quiet columns of sample n, bias = 0.1 randn; k[n, g] is solved so that the group's float64
mean / std is its signed class.  (With iid inputs on every channel and one k per group, mean / std could not pass ~ sqrt(Cin), and
the second sample could not differ from the first.)  No dead group: a row of zero weights says nothing about the GEMM.

RESTATEMENT.  Conv2d 1x1 + GroupNorm, eps 1e-5: float64 (the yardstick, group_norm64) and F.conv2d + F.group_norm in float32 on the CPU.  study(case) computes both once."""
import functools

import torch
import torch.nn.functional as F

CLASSES = (0, 3, 10, 30, 100, 300)
DEAD = "dead"
GROUPS = 32
EPS = 1e-5
DEAD_GROUP = 7            # a class-3 slot of sample 0 (class 0 and class 3 have six groups per sample: five stay)
DEAD_VALUE = -200.0
FACTOR = 8.0              # the project's standing factor over the float32 restatement
DRAWN_TOL = 2e-5          # test_conv1x1_groupnorm_unit's bound, here per class.  The margin is thin where fp32 arithmetic itself is near it: drawn-2x1075x2048x256,
                          # token rows in, class 100 measures 1.94e-5 on the device (the float32 restatement 1.6e-5).  The kernels are bit-deterministic, so it holds
                          # run after run; another summation order in that GEMM path (split-K, k-step order) can move it past the bound without being wrong.

# (N, HW, Cin, Cout): the smallest shapes that reach each branch
SHAPES = [(2, 1, 32, 64),         # one pixel, cg = 2
          (2, 63, 32, 96),        # cg = 3: a float4 straddles groups, 24 lanes x 10 row groups
          (2, 64, 32, 384),       # cg = 12
          (2, 65, 64, 256),       # a second block of one row: the most unequal block weights
          (2, 130, 32, 192),      # cg = 6, ragged third block
          (2, 16, 32, 512),
          (2, 100, 32, 1024),     # lanes = 256, RG = 1
          (2, 35, 256, 2048),     # two channel-loop passes, cg = 64: one group per 64-channel apply block
          (2, 1075, 64, 256),     # 25 x 43
          (1, 4161, 32, 64),      # 66 blocks: past the 64-lane stride
          (1, 32833, 32, 64)]     # 514 blocks: past the 8-deep batch
SPLITK_SHAPE = (2, 1075, 2048, 256)      # drawn family only: the split-K path
EXACT_SUMS_HW = 130       # up to here every fp32 sum of the dead group's constant is exact


def signed_classes(n):
    """[(class, sign)] per group for sample n"""
    lst = [(CLASSES[g % 6], -1.0 if (g // 6) % 2 else 1.0) for g in range(GROUPS)]
    return lst if n == 0 else lst[::-1]


class Case:
    def __init__(self, family, shape, x, w, b, gamma, beta, dead):
        self.family, self.shape = family, tuple(shape)
        self.N, self.HW, self.Cin, self.Cout = self.shape
        self.cg = self.Cout // GROUPS
        self.x, self.w, self.b, self.gamma, self.beta = (t.float().contiguous() for t in (x, w, b, gamma, beta))
        self.dead = dead          # group index or None
        self.name = f"{family}-{'x'.join(str(v) for v in shape)}"

    def label(self, n, g):
        return DEAD if g == self.dead else signed_classes(n)[g][0]

    def labels(self):
        return [c for c in CLASSES + (DEAD,) if any(self.label(n, g) == c for n in range(self.N) for g in range(GROUPS))]

    def __repr__(self):
        return self.name


QUANT = 2.0 ** -10        # bias and switch are multiples of this (a one-pixel group's std is a few 1/128: 1/64 would be too coarse to place a class)


def _rq(t):
    return torch.round(t / QUANT) * QUANT


def _sig8(t):
    """round to 8 significant bits (exact in bf16), keeping multiples of QUANT"""
    e = torch.floor(torch.log2(t.abs().clamp_min(QUANT)))
    q = torch.maximum(2.0 ** (e - 7), torch.tensor(QUANT, dtype=t.dtype))
    return torch.round(t / q) * q


@functools.lru_cache(maxsize=None)
def exact_case(shape):
    N, HW, Cin, Cout = shape
    cg = Cout // GROUPS
    o = torch.arange(Cout)
    grp = o // cg
    w = torch.zeros(Cout, Cin, dtype=torch.float64)
    for k in range(4):
        ch = 2 + (o * 5 + 9 * k + o // 7) % (Cin - 2)            # 9 k mod (Cin - 2) differ for k = 0..3 at Cin = 32, 64, 256
        w[o, ch] = 1.0 - 2.0 * ((o >> k) & 1).double()
    w[grp == DEAD_GROUP] = 0.0
    live = torch.arange(GROUPS) != DEAD_GROUP
    for seed in range(7100 + HW + Cout, 7200 + HW + Cout):      # the first draw on which no live group is (nearly) constant: one pixel of two channels can be
        gen = torch.Generator().manual_seed(seed)
        x = torch.randint(-64, 65, (N, Cin, HW), generator=gen).double() / 64.0
        for n in range(N):
            x[n, :2] = float(n)
        z = torch.einsum("oc,ncp->nop", w, x) + ((o % cg).double() / 8.0)[None, :, None]           # the switch columns are still zero
        zg = z.reshape(N, GROUPS, cg * HW)
        mean, std = zg.mean(-1), zg.std(-1, unbiased=False)
        if float(std[:, live].min()) >= 1 / 16:
            break
    else:
        raise AssertionError("no usable draw")
    want = [torch.tensor([c * s for c, s in signed_classes(n)], dtype=torch.float64) * std[n] - mean[n] for n in range(N)]
    off0 = _rq(want[0])
    b = off0[grp] + (o % cg).double() / 8.0
    if N > 1:
        sw = _rq(want[1] - off0)
        hi = _sig8(sw)
        w[:, 0], w[:, 1] = hi[grp], _sig8(sw - hi)[grp]
    dead = grp == DEAD_GROUP
    w[dead] = 0.0
    b[dead] = DEAD_VALUE
    gamma = 1.0 + (o % 5).double() / 8.0
    beta = (o % 3).double() / 4.0 - 0.25
    return Case("exact", shape, x, w, b, gamma, beta, DEAD_GROUP)


def _solve_k(target, m0, v0, cov, mt, vt):
    """k with (m0 + k mt) / sqrt(v0 + 2 k cov + k^2 vt) = target (mt > 0): bisection on the side of target's sign"""
    if target == 0:
        return -m0 / mt
    f = lambda k: (m0 + k * mt) / max(v0 + 2 * k * cov + k * k * vt, 1e-300) ** 0.5
    lo, hi = -m0 / mt, -m0 / mt + (1.0 if target > 0 else -1.0)
    while abs(f(hi)) < abs(target):
        hi = lo + 2.0 * (hi - lo)
        assert abs(hi) < 1e9, "class out of reach"
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if abs(f(mid)) < abs(target):
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


@functools.lru_cache(maxsize=None)
def drawn_case(shape):
    N, HW, Cin, Cout = shape
    cg = Cout // GROUPS
    gen = torch.Generator().manual_seed(9000 + HW + Cin + Cout)
    c = torch.arange(Cin)
    x = torch.relu(torch.randn(N, Cin, HW, generator=gen) + 0.5)
    quiet = torch.relu(0.5 + torch.randn(N, Cin, HW, generator=gen) / 1024.0)
    for n in range(2):
        lit = c % 4 == (1 if n == 0 else 3)
        if n < N:
            x[n, lit] = quiet[n, lit]
        for m in range(N):
            if m != n:
                x[m, lit] = 0.0
    w = torch.randn(Cout, Cin, generator=gen) / Cin ** 0.5
    b = 0.1 * torch.randn(Cout, generator=gen)
    gamma = 1.0 + 0.1 * torch.randn(Cout, generator=gen)
    beta = 0.1 * torch.randn(Cout, generator=gen)
    x64, w64 = x.double(), w.double()
    for n in range(N):
        lit = c % 4 == (1 if n == 0 else 3)
        y0 = (torch.einsum("oc,cp->op", w64, x64[n]) + b.double()[:, None]).reshape(GROUPS, cg, HW)
        t = x64[n, lit].sum(0) / Cin                      # what one unit of k adds to every channel of the group, per pixel
        mt, vt = float(t.mean()), float(t.var(unbiased=False))
        for g, (cls, sign) in enumerate(signed_classes(n)):
            m0, v0 = float(y0[g].mean()), float(y0[g].var(unbiased=False))
            cov = float(((y0[g] - m0) * (t - mt)[None, :]).mean())
            k = _solve_k(sign * cls, m0, v0, cov, mt, vt)
            w64[g * cg:(g + 1) * cg, lit] += k / Cin
    return Case("drawn", shape, x, w64.float(), b, gamma, beta, None)


def exact_cases():
    return [exact_case(s) for s in SHAPES]


def drawn_cases():
    return [drawn_case(s) for s in SHAPES + [SPLITK_SHAPE]]


def conv64(case):
    return torch.einsum("oc,ncp->nop", case.w.double(), case.x.double()) + case.b.double()[None, :, None]


def measured_ratio(case, y64):
    """[N][G] mean / std of y in float64 (inf where the group is constant)"""
    yg = y64.reshape(case.N, GROUPS, -1)
    return yg.mean(-1) / yg.std(-1, unbiased=False)


def group_norm64(y64, case):
    """The yardstick: GroupNorm as written, (y - mean) / sqrt(var + eps) * gamma + beta, two passes in float64.  (F.group_norm evaluates
    y * (rstd gamma) + (beta - mean rstd gamma): the same function, but its rounding grows with |mean| rstd -- 1e-11 on the dead group in float64,
    r 2^-24 in float32, which is the float32 restatement's error below.)"""
    yg = y64.reshape(case.N, GROUPS, case.cg, -1)
    mean = yg.mean((2, 3), keepdim=True)
    var = ((yg - mean) ** 2).mean((2, 3), keepdim=True)
    out = (yg - mean) / torch.sqrt(var + EPS)
    return out.reshape(y64.shape) * case.gamma.double()[None, :, None] + case.beta.double()[None, :, None]


class Study:
    """y64 [N, Cout, HW]; ref64, ref32: the restatements' outputs, NCHW; err32 = class_err(ref32, ref64)"""


@functools.lru_cache(maxsize=None)
def study(case):
    s = Study()
    s.y64 = conv64(case)
    s.ref64 = group_norm64(s.y64, case)
    y32 = F.conv2d(case.x[:, :, :, None], case.w[:, :, None, None], case.b)[..., 0]
    s.y32 = y32
    s.ref32 = F.group_norm(y32, GROUPS, case.gamma, case.beta, EPS)
    s.err32 = class_err(case, s.ref32, s.ref64)
    s.scale = class_scale(case, s.ref64)
    return s


def _per_class(case, per_block):
    """per_block [N][G] -> {label: max over the label's (sample, group) blocks}"""
    out = {}
    for n in range(case.N):
        for g in range(GROUPS):
            lab = case.label(n, g)
            out[lab] = max(out.get(lab, 0.0), float(per_block[n, g]))
    return out


def class_err(case, got, want):
    """got, want [N, Cout, HW] -> {class: max over its (sample, group) blocks of max |got - want|}; NaN / inf count as inf"""
    d = (got.double().cpu() - want.double()).abs().reshape(case.N, GROUPS, -1)
    d = torch.where(torch.isfinite(d), d, torch.full_like(d, float("inf")))
    return _per_class(case, d.amax(-1))


def class_scale(case, want):
    return _per_class(case, want.double().abs().reshape(case.N, GROUPS, -1).amax(-1))


def param_class_err(case, got, want):
    """per-channel tensors [Cout] (d_gn_w, d_gn_b): {class of sample 0's group: (max |got - want|, max |want|)}"""
    d = (got.double().cpu() - want.double()).abs().reshape(GROUPS, -1).amax(-1)
    s = want.double().abs().reshape(GROUPS, -1).amax(-1)
    out = {}
    for g in range(GROUPS):
        lab = case.label(0, g)
        e, m = out.get(lab, (0.0, 0.0))
        out[lab] = (max(e, float(d[g])), max(m, float(s[g])))
    return out


def ulp32(v):
    """spacing of fp32 numbers at |v|"""
    t = torch.tensor(abs(float(v)), dtype=torch.float32)
    return float(torch.nextafter(t, torch.tensor(float("inf"))) - t)


def bound(case, st, label):
    """exact family: 8 x the float32 restatement's class error; the dead group: at least one ulp of its constant through the normalisation"""
    b = FACTOR * st.err32[label]
    if label == DEAD:
        b = max(b, EPS ** -0.5 * ulp32(DEAD_VALUE) * float(case.gamma.abs().max()))
    return b


def drawn_classes_asserted(case):
    """The classes of a drawn case held to DRAWN_TOL on the device: all of them, but for the top one where the float32 restatement itself (an fp32
    convolution's rounding of a mean of 300 standard deviations) is not under DRAWN_TOL / 8 there.  Never more than the top class."""
    st = study(case)
    top = CLASSES[-1]
    fair = st.err32[top] / st.scale[top] < DRAWN_TOL / FACTOR
    return [lab for lab in case.labels() if lab != top or fair]


def report(tag, case, err, st):
    """one line per class: error, restatement error, ratio"""
    lines = []
    for lab in case.labels():
        r = st.err32[lab]
        lines.append(f"{tag:<28} {case.name:<26} class {str(lab):>4}  err {err[lab]:.3e}  float32 restatement {r:.3e}  ratio {err[lab] / r if r > 0 else float('inf') if err[lab] > 0 else 0.0:.2f}")
    return lines


# ---- fp32 restatements of summation orders (test code: what the orders do to the statistics, not the kernels' text) ----
def _pad_rows(y, mult):
    """y [HW, C] -> zero rows appended up to a multiple of `mult`; valid [HWp] mask"""
    HW = y.shape[0]
    HWp = -(-HW // mult) * mult
    yp = torch.zeros(HWp, y.shape[1], dtype=y.dtype)
    yp[:HW] = y
    valid = torch.zeros(HWp, dtype=y.dtype)
    valid[:HW] = 1.0
    return yp, valid


def _seq_sum(t, dim):
    """fp32 sum along dim in index order"""
    acc = torch.zeros_like(t.select(dim, 0))
    for i in range(t.shape[dim]):
        acc = acc + t.select(dim, i)
    return acc


def _lanes_then_butterfly(t):
    """t [nblk, ...]: 64 lanes stride over the blocks in order, then an xor butterfly (32 .. 1); lane 0's value"""
    nblk = t.shape[0]
    k = -(-nblk // 64)
    tp = torch.zeros((k * 64,) + t.shape[1:], dtype=t.dtype)
    tp[:nblk] = t
    lanes = _seq_sum(tp.reshape((k, 64) + t.shape[1:]), 0)
    idx = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[idx ^ o]
    return lanes[0]


def _row_groups(C):
    n4 = C // 4
    lanes = min(n4, 256)
    return 256 // lanes


def _thread_split(y, C):
    """y [HW, C] fp32 -> v [nblk, I, RG, C] (row j + RG i of block b), valid [nblk, I, RG, 1], rows per block [nblk]"""
    RG = _row_groups(C)
    HW = y.shape[0]
    nblk = -(-HW // 64)
    yp, valid = _pad_rows(y, 64)
    I = -(-64 // RG)
    v = torch.zeros(nblk, I * RG, C)
    m = torch.zeros(nblk, I * RG)
    v[:, :64] = yp.reshape(nblk, 64, C)
    m[:, :64] = valid.reshape(nblk, 64)
    rows = m.sum(1)
    return v.reshape(nblk, I, RG, C), m.reshape(nblk, I, RG, 1), rows, RG


def stats_eval_raw(y, cg):
    """The eval kernels' order before the fix, fp32: 64-row blocks; per (row group, channel) sums of y and y^2 over rows j, j + RG, ..;
    per group: row groups then channels; blocks: lanes + butterfly; var = q / cnt - mu * mu.  y [HW, C] -> (mean [G], rstd [G])"""
    HW, C = y.shape
    v, m, rows, RG = _thread_split(y, C)
    s, q = _seq_sum(v, 1), _seq_sum(v * v, 1)                                  # [nblk, RG, C]
    G = C // cg
    s = _seq_sum(s.reshape(-1, RG, G, cg).permute(0, 2, 1, 3).reshape(-1, G, RG * cg), 2)
    q = _seq_sum(q.reshape(-1, RG, G, cg).permute(0, 2, 1, 3).reshape(-1, G, RG * cg), 2)
    s, q = _lanes_then_butterfly(s), _lanes_then_butterfly(q)
    cnt = torch.tensor(float(HW * cg))
    mu = s / cnt
    return mu, 1.0 / torch.sqrt(torch.clamp(q / cnt - mu * mu, min=0.0) + torch.tensor(EPS))


def stats_train_raw(y, cg):
    """The training tier's order before the fix: fp32 per (block, channel) sums of y and y^2 over the 64 rows, blocks in order, then float64 over
    the channels of a group and float64 E[y^2] - mean^2"""
    HW, C = y.shape
    yp, _ = _pad_rows(y, 64)
    v = yp.reshape(-1, 64, C)
    s, q = _seq_sum(_seq_sum(v, 1), 0), _seq_sum(_seq_sum(v * v, 1), 0)       # [C]
    G = C // cg
    s, q = s.double().reshape(G, cg).sum(1), q.double().reshape(G, cg).sum(1)
    cnt = float(HW * cg)
    mu = s / cnt
    var = torch.clamp(q / cnt - mu * mu, min=0.0)
    return mu.float(), (1.0 / torch.sqrt(var + EPS)).float()


def stats_eval_centred(y, cg):
    """THE ORDER THE FIX USES in the eval path (gn_stats_kernel, gn_apply_kernel's prologue), fp32 throughout.  Every level carries
    (count, mean, M2 about its own mean); a parent is, with ref = its first child's mean,
          mean = ref + sum n_i (mean_i - ref) / n,    M2 = sum_i M2_i + n_i (mean_i - mean)^2
    so that no sum runs over mean-sized terms: the mean is rounded at its own size once per level.
      thread (row group j, channel) of a 64-row block: one sweep over rows j, j + RG, .. with its first row y0 as the reference:
            a = sum (y - y0), q = sum (y - y0)^2, mean = y0 + a / n, M2 = q - a^2 / n
      block, per group: row groups then channels -> (mean_b, M2_b)
      group: the blocks by lanes + butterfly, about block 0's mean -> mean; then M2 the same way; rstd = rsqrt(M2 / cnt + eps)"""
    HW, C = y.shape
    v, m, rows, RG = _thread_split(y, C)
    nj = m.sum(1)                                                              # [nblk, RG, 1] rows of the thread
    inv = 1.0 / nj.clamp_min(1.0)
    d = (v - v[:, :1]) * m
    a, q = _seq_sum(d, 1), _seq_sum(d * d, 1)
    mt = v[:, 0] + a * inv
    m2t = torch.clamp(q - a * a * inv, min=0.0)
    G = C // cg
    grp = lambda t: t.reshape(-1, RG, G, cg).permute(0, 2, 1, 3).reshape(-1, G, RG * cg)
    njg, mtg = grp(nj.expand(-1, -1, C)), grp(mt)                              # (entries of a thread without rows have n = 0)
    nb = (rows * cg)[:, None]
    ref = mtg[:, :, :1]
    mub = ref[:, :, 0] + _seq_sum(njg * (mtg - ref), 2) / nb
    dd = mtg - mub[:, :, None]
    m2b = _seq_sum(torch.where(njg > 0, grp(m2t) + njg * dd * dd, torch.zeros(())), 2)        # [nblk, G]
    cnt = torch.tensor(float(HW * cg))
    mu = mub[0] + _lanes_then_butterfly(nb * (mub - mub[:1])) / cnt
    db = mub - mu[None, :]
    m2 = _lanes_then_butterfly(m2b + nb * db * db)
    return mu, 1.0 / torch.sqrt(m2 / cnt + torch.tensor(EPS))


def stats_train_centred(y, cg):
    """THE ORDER THE FIX USES in the training tier, the same merge: per (block, channel) one fp32 sweep over the 64 rows with the block's first row as the
    reference -> (mean, M2); blocks merged per channel in block order about block 0's mean, fp32 (gt_merge_blocks_kernel); channels merged per group in
    float64 (gt_group_stats_kernel)"""
    HW, C = y.shape
    yp, valid = _pad_rows(y, 64)
    v, m = yp.reshape(-1, 64, C), valid.reshape(-1, 64, 1)
    rows = m.sum(1)                                                            # [nblk, 1]
    d = (v - v[:, :1]) * m
    a, q = _seq_sum(d, 1), _seq_sum(d * d, 1)                                  # [nblk, C]
    inv = 1.0 / rows
    mb = v[:, 0] + a * inv
    m2b = torch.clamp(q - a * a * inv, min=0.0)
    muc = mb[0] + _seq_sum(rows * (mb - mb[:1]), 0) / torch.tensor(float(HW))
    dd = mb - muc[None, :]
    m2c = _seq_sum(m2b + rows * dd * dd, 0)                                    # [C]
    G = C // cg
    mu = muc.double().reshape(G, cg).sum(1) / cg
    dc = muc.double().reshape(G, cg) - mu[:, None]
    m2 = (m2c.double().reshape(G, cg) + HW * dc * dc).sum(1)
    return mu.float(), (1.0 / torch.sqrt(m2 / float(HW * cg) + EPS)).float()


def apply_fp32(y, mu, rstd, gamma, beta, cg):
    """(y - mean) rstd gamma + beta in fp32; y [HW, C] -> [C, HW]"""
    mu_c, rs_c = mu.repeat_interleave(cg), rstd.repeat_interleave(cg)
    return (((y - mu_c[None, :]) * rs_c[None, :]) * gamma[None, :] + beta[None, :]).t()


def restate(case, y32, stats):
    """The normalised output [N, Cout, HW] of a summation order on the fp32 conv output y32 [N, Cout, HW]"""
    outs = []
    for n in range(case.N):
        y = y32[n].t().contiguous()
        mu, rs = stats(y, case.cg)
        outs.append(apply_fp32(y, mu, rs, case.gamma, case.beta, case.cg))
    return torch.stack(outs)
