"""Per-element checks of the multi-scale deformable attention sampling op: an independent float64 reference with a derived error band,
a float32 restatement of the kernel arithmetic with switchable mutations, and the case generators that put samples where the kernels
branch (tests/test_msda_sampling_cpu.py, tests/test_hip_msda_sampling.py).

LOCATION CONVENTION (one for the whole suite; golden_util.msda_core_inputs draws in it too): sampling_locations[..., 0] is x, [..., 1] is
y, both normalised to [0, 1] over the level's map, so the pixel coordinate of a sample on a level of H x W pixels is
    x = loc_x * W - 0.5,    y = loc_y * H - 0.5
and pixel (row i, column j) has its centre at loc = ((j + 0.5) / W, (i + 0.5) / H).  A sample contributes iff -1 < x < W and
-1 < y < H (strict); x0 = floor(x), lw = x - x0, hw = 1 - lw (lh, hh in y); the four corners (y0, x0), (y0, x0 + 1), (y0 + 1, x0),
(y0 + 1, x0 + 1) carry w1 = hh hw, w2 = hh lw, w3 = lh hw, w4 = lh lw and count only where they lie on the map.  With g = grad_output:
    out[n, q, m, d]            = sum_{l, p} attn (w1 v1 + w2 v2 + w3 v3 + w4 v4)
    grad_value[corner row][d] += w_corner attn g[d]
    grad_attn[l, p]            = sum_d g[d] (w1 v1 + w2 v2 + w3 v3 + w4 v4)
    grad_loc[l, p]             = sum_d attn g[d] (W (-hh v1 + hh v2 - lh v3 + lh v4),  H (-hw v1 - lw v2 + hw v3 + lw v4))
(the comment above msda_core_bwd_kernel, axial_vs_amd/csrc/axvs_msda.h).  The derivative is the floor-side one where x is an integer.

THE BAND.  reference() evaluates these sums in float64 on the float32 input values with explicit index arithmetic and index_add_, level
by level, and returns for each of the four results
    ref   the float64 value,
    n     the number of terms added into the element (grad_value: the contributions to that value element, from scattering ones),
    mag0  the same sum with every term replaced by its absolute value,
    mag   mag0 with every bilinear factor enlarged by the coordinate rounding  delta = eps32 (|x| + |y| + 1)  -- what computing
          loc * W - 0.5 in fp32 can move x by, hence lw and hw -- and, where a factor is below delta (the coordinate is within fp32
          rounding of an integer, so fp32 and float64 may floor differently or disagree on -1 < x < W), a factor delta on the
          neighbouring pixel the other floor would have used.
An fp32 sum of n products of a few factors, in any order (that covers the atomics), is within eps32 (n + 8) mag0 of the exact sum of
the SAME products.  The products are not the same: the fp32 coordinate differs from the float64 one by up to delta, which moves every
bilinear weight by delta ABSOLUTELY -- not by eps32 of itself -- so the sum moves by up to  mag - mag0.  The band is therefore

    |got - ref| <= eps32 (n + 8) mag + (mag - mag0)

The first statement of this check had only the first term (with the delta-enlarged mag): that multiplies the coordinate rounding by
eps32 a second time, and the float32 restatement below leaves it where few products share an element (85-pixel-wide map, one
sample per query: 17x on out, 1000x on grad_value; test_msda_sampling_cpu.test_coordinate_rounding_needs_its_own_term).  The second term is derived, not fitted: it is
zero where coordinates are exact (the lattice cases), and a few eps32 |x| |attn v| elsewhere.
grad_sampling_loc jumps where a pixel coordinate is an integer, so on randomly drawn cases samples with a coordinate within KINK px of
an integer are left out of that one tensor (`near`); nothing is left out on exact (lattice) cases or of any other tensor."""
import math

import torch

EPS32 = 2.0 ** -23
KINK = 1e-3          # px; fp32 coordinate rounding at W <= 160 is ~1e-5 px
MAX_EXCLUDED = 0.02  # share of grad_sampling_loc samples that may be left out on random cases (uniform locations: ~0.4 %)
TENSORS = ("out", "grad_value", "grad_sampling_loc", "grad_attn_weight")


class Case:
    """One call of the op.  value [N,S,M,D], loc [N,Lq,M,L,P,2], aw [N,Lq,M,L,P], gout [N,Lq,M*D], all float32.
    exact: the pixel coordinates are exactly representable and loc * W - 0.5 is exact in fp32 (nothing excluded)."""

    def __init__(self, name, family, shapes, value, loc, aw, gout, exact=False):
        self.name, self.family, self.shapes, self.exact = name, family, [(int(h), int(w)) for h, w in shapes], exact
        self.value, self.loc, self.aw, self.gout = value.float().contiguous(), loc.float().contiguous(), aw.float().contiguous(), gout.float().contiguous()
        N, S, M, D = self.value.shape
        assert S == sum(h * w for h, w in self.shapes) and self.loc.shape[:3] == (N, self.loc.shape[1], M) and self.loc.shape[3] == len(self.shapes)
        assert self.aw.shape == self.loc.shape[:-1] and self.gout.shape == (N, self.loc.shape[1], M * D)

    @property
    def dims(self):
        N, S, M, D = self.value.shape
        _, Lq, _, L, P, _ = self.loc.shape
        return N, S, M, D, Lq, L, P

    def __repr__(self):
        return self.name


class Result:
    def __init__(self, ref, n=None, mag0=None, mag=None):
        self.ref, self.n, self.mag0, self.mag = ref, n, mag0, mag

    def band(self, coord=True):
        b = EPS32 * (self.n + 8.0) * self.mag
        return b + (self.mag - self.mag0) if coord else b


class _Acc:
    """the four sums: out [G, D], grad_attn / grad_loc x / y [G L P], grad_value [N S M, D]"""

    def __init__(self, G, LP, R, D, dtype, backward=True, counts=False, device="cpu"):
        self.backward = backward
        self.out = torch.zeros(G, D, dtype=dtype, device=device)
        self.ga, self.gx, self.gy = (torch.zeros(G * LP, dtype=dtype, device=device) for _ in range(3))
        self.gv = torch.zeros(R, D, dtype=dtype, device=device) if backward else None
        self.n = [torch.zeros(k, dtype=torch.float64, device=device) for k in (G, G * LP, R)] if counts else None

    def add(self, grp, slot, row, v, a, g, w, cx, cy):
        """terms of one corner for the listed samples: group, sample slot, value row, v [K, D], attn, g [K, D], weight, d weight / dx, / dy"""
        self.out.index_add_(0, grp, (a * w)[:, None] * v)
        if self.n is not None:
            one = torch.ones(grp.numel(), dtype=torch.float64, device=grp.device)
            self.n[0].index_add_(0, grp, one)
            self.n[1].index_add_(0, slot, one * v.shape[1])
            self.n[2].index_add_(0, row, one)
        if not self.backward:
            return
        gv = (g * v).sum(-1)
        self.ga.index_add_(0, slot, w * gv)
        self.gx.index_add_(0, slot, a * cx * gv)
        self.gy.index_add_(0, slot, a * cy * gv)
        self.gv.index_add_(0, row, (a * w)[:, None] * g)


MUTATIONS = ("x_lt_W_to_le_W_minus_1", "x_gt_minus_1_to_ge_0", "right_corner_needs_W_minus_1", "floor_to_round", "floor_to_trunc",
             "grad_loc_scale_H_W_swapped", "lw_hw_swapped_in_one_corner", "level_start_off_by_one_row", "attn_weight_of_neighbour_point",
             "d0_store_skipped_for_last_sample")


def _sums(case, dtype, backward=True, mut=None, mags=False, device="cpu"):
    """The op level by level in `dtype`.  mut: one of MUTATIONS (float32 restatement only).  mags: also the magnitude sums and counts."""
    N, S, M, D, Lq, L, P = case.dims
    G, LP, R = N * Lq * M, L * P, N * S * M
    vflat = case.value.to(device, dtype).reshape(R, D)
    loc = case.loc.to(device, dtype).reshape(G, L, P, 2)
    aw = case.aw.to(device, dtype).reshape(G, L, P)
    gout = case.gout.to(device, dtype).reshape(G, D)
    ar = lambda k: torch.arange(k, device=device)
    grp_all = ar(G).view(G, 1).expand(G, P).reshape(-1)
    base = (ar(N).view(N, 1, 1) * (S * M) + ar(M).view(1, 1, M)).expand(N, Lq, M).reshape(G, 1).expand(G, P).reshape(-1)
    acc = _Acc(G, LP, R, D, dtype, backward, counts=mags, device=device)
    m0 = _Acc(G, LP, R, D, dtype, backward, device=device) if mags else None
    m1 = _Acc(G, LP, R, D, dtype, backward, device=device) if mags else None
    near = torch.zeros(G, L, P, dtype=torch.bool, device=device)
    dead = torch.zeros(G, L, P, dtype=torch.bool, device=device)
    start = 0
    for l, (H, W) in enumerate(case.shapes):
        slot_all = (ar(G).view(G, 1) * LP + l * P + ar(P).view(1, P)).reshape(-1)
        x = (loc[:, l, :, 0] * W - 0.5).reshape(-1)
        y = (loc[:, l, :, 1] * H - 0.5).reshape(-1)
        a = aw[:, l].reshape(-1)
        if mut == "attn_weight_of_neighbour_point":
            a = aw[:, l].roll(-1, dims=-1).reshape(-1)
        x_hi = (x <= W - 1) if mut == "x_lt_W_to_le_W_minus_1" else (x < W)
        x_lo = (x >= 0) if mut == "x_gt_minus_1_to_ge_0" else (x > -1)
        inr = x_lo & x_hi & (y > -1) & (y < H)
        # dead samples are parked on pixel 0 (their floats may be 1e31: no index is taken from them)
        alive = (x > -2) & (x < W + 1) & (y > -2) & (y < H + 1)
        use = alive if mags else inr
        xs, ys = torch.where(use, x, torch.zeros_like(x)), torch.where(use, y, torch.zeros_like(y))
        fl = torch.round if mut == "floor_to_round" else torch.trunc if mut == "floor_to_trunc" else torch.floor
        xf, yf = fl(xs), fl(ys)
        lw, lh = xs - xf, ys - yf
        hw, hh = 1 - lw, 1 - lh
        x0, y0 = xf.long(), yf.long()
        sx, sy = (H, W) if mut == "grad_loc_scale_H_W_swapped" else (W, H)
        lstart = start - W if (mut == "level_start_off_by_one_row" and l > 0) else start
        wright = W - 1 if mut == "right_corner_needs_W_minus_1" else W

        def rows(sel, yi, xi):
            return base[sel] + (lstart + yi[sel] * W + xi[sel]) * M

        # (dy, dx, weight, d weight / dx, d weight / dy): w1 .. w4 in the kernel's order
        c2w = hh * hw if mut == "lw_hw_swapped_in_one_corner" else hh * lw
        corners = ((0, 0, hh * hw, -hh, -hw), (0, 1, c2w, hh, -lw), (1, 0, lh * hw, -lh, hw), (1, 1, lh * lw, lh, lw))
        for dy, dx, w, cx, cy in corners:
            yi, xi = y0 + dy, x0 + dx
            onmap = (yi >= 0) & (yi < H) & (xi >= 0) & (xi < (wright if dx else W))
            sel = (inr & onmap).nonzero().squeeze(1)
            if sel.numel():
                row = rows(sel, yi, xi)
                acc.add(grp_all[sel], slot_all[sel], row, vflat[row], a[sel], gout[grp_all[sel]], w[sel], sx * cx[sel], sy * cy[sel])
                if mags:
                    m0.add(grp_all[sel], slot_all[sel], row, vflat[row].abs(), a[sel].abs(), gout[grp_all[sel]].abs(), w[sel].abs(), W * cx[sel].abs(),
                           H * cy[sel].abs())
        if mags:
            delta = EPS32 * (xs.abs() + ys.abs() + 1) * (0.0 if case.exact else 1.0)      # exact coordinates do not round
            din = inr.to(dtype)            # (the derivative terms belong to samples inside the strict bounds)
            # per axis: (offset, magnitude of the factor, magnitude of its derivative); the outer taps exist only within delta of an integer
            tx = ((-1, delta * (lw < delta), 0 * lw), (0, hw + delta, din), (1, lw + delta, din), (2, delta * (hw < delta), 0 * lw))
            ty = ((-1, delta * (lh < delta), 0 * lh), (0, hh + delta, din), (1, lh + delta, din), (2, delta * (hh < delta), 0 * lh))
            edge = alive & ((lw < delta) | (hw < delta) | (lh < delta) | (hh < delta))
            for dy, wy, ddy in ty:
                for dx, wx, ddx in tx:
                    inner = dy in (0, 1) and dx in (0, 1)
                    yi, xi = y0 + dy, x0 + dx
                    sel = ((alive if inner else edge) & (yi >= 0) & (yi < H) & (xi >= 0) & (xi < W) & (wx * wy + ddx + ddy > 0)).nonzero().squeeze(1)
                    if sel.numel():
                        row = base[sel] + (start + yi[sel] * W + xi[sel]) * M
                        m1.add(grp_all[sel], slot_all[sel], row, vflat[row].abs(), a[sel].abs(), gout[grp_all[sel]].abs(), (wx * wy)[sel],
                               W * (ddx * wy)[sel], H * (wx * ddy)[sel])
            fr = torch.minimum((x - torch.round(x)).abs(), (y - torch.round(y)).abs())
            near[:, l] = (alive & (fr < KINK)).view(G, P)
            dead[:, l] = (~((x > -1 - KINK) & (x < W + KINK) & (y > -1 - KINK) & (y < H + KINK))).view(G, P)
        start += H * W
    return acc, m0, m1, near, dead


def _shape(case, acc):
    N, S, M, D, Lq, L, P = case.dims
    out = {"out": acc.out.view(N, Lq, M * D)}
    if acc.backward:
        out["grad_value"] = acc.gv.view(N, S, M, D)
        out["grad_sampling_loc"] = torch.stack([acc.gx, acc.gy], -1).view(N, Lq, M, L, P, 2)
        out["grad_attn_weight"] = acc.ga.view(N, Lq, M, L, P)
    return out


def reference(case, backward=True, device="cpu"):
    """{tensor name: Result} in float64 on the float32 inputs, plus "near" (samples left out of grad_sampling_loc on random cases) and
    "dead" (samples further than KINK px outside -1 < x < W, -1 < y < H: every kernel must give them exactly 0.0).
    device: where torch evaluates it (the GPU file passes "cuda": the N = 4 shipped sizes take 20 s on the host, and torch's float64
    indexing kernels share nothing with the library; the CPU file checks this same code against the oracle)."""
    N, S, M, D, Lq, L, P = case.dims
    acc, m0, m1, near, dead = _sums(case, torch.float64, backward, mags=True, device=device)
    ref, mag0, mag = _shape(case, acc), _shape(case, m0), _shape(case, m1)
    n_out, n_smp, n_val = acc.n
    n = {"out": n_out.view(N, Lq, M, 1).expand(N, Lq, M, D).reshape(N, Lq, M * D), "grad_value": n_val.view(N, S, M, 1).expand(N, S, M, D),
         "grad_sampling_loc": n_smp.view(N, Lq, M, L, P, 1).expand(N, Lq, M, L, P, 2), "grad_attn_weight": n_smp.view(N, Lq, M, L, P)}
    res = {k: Result(ref[k], n[k], mag0[k], torch.maximum(mag[k], mag0[k])) for k in ref}
    res["near"] = torch.zeros_like(near.view(N, Lq, M, L, P)) if case.exact else near.view(N, Lq, M, L, P)
    res["dead"] = dead.view(N, Lq, M, L, P)
    return res


def restatement(case, mut=None, backward=True):
    """The kernel arithmetic in float32 on the CPU (same formulas, torch's summation order), optionally with one mutation."""
    acc, _, _, _, _ = _sums(case, torch.float32, backward, mut=mut)
    got = _shape(case, acc)
    if mut == "d0_store_skipped_for_last_sample" and backward:      # the slot keeps what the caller's buffer held
        got["grad_sampling_loc"][:, :, :, -1, -1] = float("nan")
        got["grad_attn_weight"][:, :, :, -1, -1] = float("nan")
    return got


def ratios(got, ref, coord=True):
    """{tensor: (elements checked, worst |got - ref| / band, share of samples left out)}; a NaN or an error against a zero band is inf"""
    rep = {}
    for k in TENSORS:
        if k not in got or k not in ref:
            continue
        r = ref[k]
        err = (got[k].detach().to(r.ref.device).double() - r.ref).abs()
        band = r.band(coord)
        ratio = torch.where(band > 0, err / band.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, math.inf)))
        ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, math.inf), ratio)
        share = 0.0
        if k == "grad_sampling_loc":
            keep = ~ref["near"]
            share = 1.0 - float(keep.double().mean())
            ratio = ratio[keep]
        rep[k] = (ratio.numel(), float(ratio.max()) if ratio.numel() else 0.0, share)
    return rep


def inside(rep):
    return all(w <= 1.0 and s <= MAX_EXCLUDED for _, w, s in rep.values())


def report_line(case, rep, path=""):
    parts = [f"{k} n={c} worst={w:.3f}" + (f" excluded={s:.4f}" if k == "grad_sampling_loc" else "") for k, (c, w, s) in rep.items()]
    return f"{path + ' ' if path else ''}{case.family}/{case.name}: " + "; ".join(parts)


# ---- case generators ----------------------------------------------------------------------------------------------------------------
def _values(g, N, S, M, D, Lq, wide=False):
    value, gout = torch.randn(N, S, M, D, generator=g), torch.randn(N, Lq, M, D, generator=g)
    if wide:       # magnitudes 1e-6 .. 1e3 across channels, mixed sign
        sc = 10.0 ** torch.linspace(-6, 3, max(D, 2))[:D]
        value, gout = value * sc, gout * sc.flip(0) if D > 1 else gout
    return value, gout.reshape(N, Lq, M * D)


def _from_px(name, family, shapes, px, D, seed, aw=None, exact=False, wide=False):
    """px [N,Lq,M,L,P,2] pixel coordinates (x, y), float64 -> loc = (px + 0.5) / (W, H)"""
    g = torch.Generator().manual_seed(seed)
    N, Lq, M, L, P, _ = px.shape
    wh = torch.tensor([[w, h] for h, w in shapes], dtype=torch.float64).view(1, 1, 1, L, 1, 2)
    loc = ((px.double() + 0.5) / wh).float()
    if exact:
        back = loc.double() * wh - 0.5
        assert torch.equal(back.float().double(), back) and torch.equal(back, px.double()), name
    S = sum(h * w for h, w in shapes)
    value, gout = _values(g, N, S, M, D, Lq, wide)
    if aw is None:
        aw = torch.rand(N, Lq, M, L, P, generator=g) + 0.05
    return Case(name, family, shapes, value, loc, aw, gout, exact)


LATTICE_SHAPES = [(8, 16), (1, 8), (16, 1), (1, 1)]


def _edge_values(W):
    e = 2.0 ** -10
    return [-1.0, -1 + e, -0.5, 0.0, W - 1.0, W - 1 + e, W - e, float(W), W + 3.0, min(3, W - 1) * 1.0, min(3, W - 1) - 0.5, 1e4, -1e4]


def lattice():
    """dyadic pixel coordinates on power-of-two maps: loc * W - 0.5 is exact in fp32, both sides take the floor-side derivative"""
    cases = []
    L = len(LATTICE_SHAPES)
    K = len(_edge_values(8))
    px = torch.zeros(1, K * K, 2, L, 1, 2, dtype=torch.float64)
    for l, (H, W) in enumerate(LATTICE_SHAPES):
        xs, ys = torch.tensor(_edge_values(W), dtype=torch.float64), torch.tensor(_edge_values(H), dtype=torch.float64)
        pair = torch.stack([xs.view(1, K).expand(K, K), ys.view(K, 1).expand(K, K)], -1).reshape(K * K, 2)
        px[0, :, 0, l, 0] = pair
        px[0, :, 1, l, 0] = pair.roll(7 + l, 0)          # the second head meets the pairings in another order
    c = _from_px("all_pairings_L4_P1", "lattice", LATTICE_SHAPES, px, 4, 11, exact=True)
    c.loc[0, 3, 0, 0, 0, 0], c.loc[0, 5, 1, 0, 0, 1], c.loc[0, 9, 0, 1, 0] = 1e30, -1e30, torch.tensor([-1e30, 1e30])
    cases.append(c)
    cases.append(_from_px("all_pairings_8x16_D3", "lattice", LATTICE_SHAPES[:1], px[:, :, :, :1], 3, 12, exact=True))
    g = torch.Generator().manual_seed(13)
    half = torch.stack([torch.stack([torch.randint(-3, 2 * W + 3, (2, 40, 2, 4), generator=g) / 2.0, torch.randint(-3, 2 * H + 3, (2, 40, 2, 4), generator=g) / 2.0], -1)
                        for H, W in LATTICE_SHAPES], 3)
    cases.append(_from_px("centres_and_halfway_L4_P4", "lattice", LATTICE_SHAPES, half, 8, 14, exact=True))
    # every sample on x == -1, x == W, y == -1 or y == H: all four results are exactly 0.0
    edges = half.clone()
    for l, (H, W) in enumerate(LATTICE_SHAPES):
        k = torch.randint(0, 4, (2, 40, 2, 4), generator=g)
        edges[:, :, :, l, :, 0] = torch.where(k == 0, torch.full_like(edges[:, :, :, l, :, 0], -1.0), torch.where(k == 1, torch.full_like(edges[:, :, :, l, :, 0], float(W)), edges[:, :, :, l, :, 0]))
        edges[:, :, :, l, :, 1] = torch.where(k == 2, torch.full_like(edges[:, :, :, l, :, 1], -1.0), torch.where(k == 3, torch.full_like(edges[:, :, :, l, :, 1], float(H)), edges[:, :, :, l, :, 1]))
    cases.append(_from_px("on_the_strict_bounds_all_zero", "lattice", LATTICE_SHAPES, edges, 8, 15, exact=True))
    return cases


BAND_SHAPES = [(7, 9), (49, 85), (25, 43), (24, 40), (12, 20)]


def _band_px(g, shapes, N, Lq, M, P):
    """random locations in the one-pixel bands (-1, 0) and (W - 1, W): the four edges and the four corners of every map"""
    px = torch.zeros(N, Lq, M, len(shapes), P, 2, dtype=torch.float64)
    for l, (H, W) in enumerate(shapes):
        kind = torch.randint(0, 8, (N, Lq, M, P), generator=g)       # 0-3: left, right, top, bottom; 4-7: corners
        u = torch.rand(N, Lq, M, P, 2, generator=g, dtype=torch.float64) * 0.998 + 0.001
        xk = torch.tensor([0, 1, 2, 2, 0, 1, 0, 1])[kind]           # 0: (-1, 0), 1: (W - 1, W), 2: anywhere inside
        yk = torch.tensor([2, 2, 0, 1, 0, 0, 1, 1])[kind]
        for ax, k, size in ((0, xk, W), (1, yk, H)):
            inner = torch.rand(N, Lq, M, P, generator=g, dtype=torch.float64) * (size - 1)
            px[:, :, :, l, :, ax] = torch.where(k == 0, u[..., ax] - 1, torch.where(k == 1, size - 1 + u[..., ax], inner))
    return px


def border_bands():
    cases = []
    for i, (D, shapes) in enumerate([(16, BAND_SHAPES[:3]), (24, BAND_SHAPES[:3]), (32, BAND_SHAPES[3:]), (1, BAND_SHAPES[:1])]):
        g = torch.Generator().manual_seed(20 + i)
        cases.append(_from_px(f"bands_D{D}_L{len(shapes)}", "border_bands", shapes, _band_px(g, shapes, 2, 40, 2, 4), D, 30 + i))
    return cases


def _uniform_px(g, shapes, N, Lq, M, P, spread):
    loc = torch.rand(N, Lq, M, len(shapes), P, 2, generator=g, dtype=torch.float64) * (1 + 2 * spread) - spread
    wh = torch.tensor([[w, h] for h, w in shapes], dtype=torch.float64).view(1, 1, 1, -1, 1, 2)
    return loc * wh - 0.5


def degenerate_maps():
    cases = []
    for i, shapes in enumerate([[(1, 5), (6, 1), (1, 1), (2, 2), (5, 7)], [(1, 7)], [(1, 1)], [(1, 5), (6, 1), (1, 1), (2, 2), (5, 7), (1, 1), (3, 4), (2, 1)]]):
        g = torch.Generator().manual_seed(40 + i)
        cases.append(_from_px(f"maps_L{len(shapes)}_{i}", "degenerate_maps", shapes, _uniform_px(g, shapes, 2, 17, 3, 2, 0.5), 8 if i % 2 == 0 else 6, 45 + i))
    return cases


SHFL_D, ATOMIC_D = (1, 2, 8, 16, 32, 64), (3, 24, 30, 48, 96)


def head_dims():
    """every D of both reduction paths; M, P and Lq cycle so that N Lq M D is mostly no multiple of 256 (a partly dead last block)"""
    cases = []
    Ms, Ps, Lqs = (1, 3, 8), (1, 3, 4, 5, 8), (1, 5, 37, 3)
    for i, D in enumerate(SHFL_D + ATOMIC_D):
        M, P, Lq, N = Ms[i % 3], Ps[i % 5], Lqs[i % 4], 1 + i % 2
        g = torch.Generator().manual_seed(50 + i)
        shapes = [(5, 7), (3, 4)]
        cases.append(_from_px(f"D{D}_M{M}_P{P}_N{N}_Lq{Lq}", "head_dims", shapes, _uniform_px(g, shapes, N, Lq, M, P, 0.2), D, 70 + i))
    g = torch.Generator().manual_seed(69)
    cases.append(_from_px("D64_M3_P4_N1_Lq5", "head_dims", [(5, 7)], _uniform_px(g, [(5, 7)], 1, 5, 3, 4, 0.2), 64, 90))    # 960 = 3.75 blocks of whole-wave groups
    return cases


def contention():
    """every query on the same point of a 4 x 4 map: Lq M P adds on four value rows (one row for the pixel-centre case)"""
    cases = []
    for i, (pt, D, Lq) in enumerate([((1.3, 2.6), 8, 4096), ((2.0, 1.0), 8, 4096), ((0.75, 0.25), 3, 512)]):
        px = torch.tensor(pt, dtype=torch.float64).view(1, 1, 1, 1, 1, 2).expand(1, Lq, 2, 1, 2, 2).contiguous()
        cases.append(_from_px(f"one_point_{pt[0]}_{pt[1]}_D{D}_Lq{Lq}", "contention", [(4, 4)], px, D, 100 + i, exact=(pt[0] % 1 == 0 or D == 3)))
    return cases


def weights():
    """attention weights that are 0, a single 1 among zeros, negative and > 1 (the op does not normalise); value and grad_output of mixed
    sign over magnitudes 1e-6 .. 1e3 across channels"""
    cases = []
    shapes = [(6, 10), (3, 5)]
    for i, D in enumerate((16, 30)):
        g = torch.Generator().manual_seed(110 + i)
        N, Lq, M, L, P = 2, 33, 3, 2, 4
        aw = torch.randn(N, Lq, M, L, P, generator=g) * 1.5
        aw = aw * (torch.rand(aw.shape, generator=g) > 0.3)
        one = torch.zeros(L * P)
        one[3] = 1.0
        aw[:, ::4] = one.view(L, P)
        cases.append(_from_px(f"signed_sparse_D{D}", "weights", shapes, _uniform_px(g, shapes, N, Lq, M, P, 0.15), D, 120 + i, aw=aw, wide=True))
    return cases


REAL = {"within_clip": [(64, 64), (32, 32), (16, 16)], "tube_link": [(48, 80), (24, 40), (12, 20)]}


def real_sizes(N=4, which=("within_clip", "tube_link"), M=8, D=32, P=4):
    """the encoder layer's own kind of call: S = Lq, the reference point is the query's pixel centre, offsets of a few pixels; the last
    point of every level is a uniform draw with spread 0.15 instead"""
    cases = []
    for i, name in enumerate(which):
        shapes = REAL[name]
        g = torch.Generator().manual_seed(130 + i)
        L, S = len(shapes), sum(h * w for h, w in shapes)
        refs = []
        for H, W in shapes:
            ys, xs = torch.meshgrid((torch.arange(H, dtype=torch.float64) + 0.5) / H, (torch.arange(W, dtype=torch.float64) + 0.5) / W, indexing="ij")
            refs.append(torch.stack([xs.reshape(-1), ys.reshape(-1)], -1))
        ref = torch.cat(refs, 0).view(1, S, 1, 1, 1, 2)
        wh = torch.tensor([[w, h] for h, w in shapes], dtype=torch.float64).view(1, 1, 1, L, 1, 2)
        px = ref * wh - 0.5 + torch.randn(N, S, M, L, P, 2, generator=g, dtype=torch.float64) * 3.0
        px[:, :, :, :, -1] = _uniform_px(g, shapes, N, S, M, 1, 0.15)[:, :, :, :, 0]
        aw = torch.softmax(torch.randn(N, S, M, L * P, generator=g), -1).view(N, S, M, L, P)
        cases.append(_from_px(f"{name}_N{N}_S{S}_M{M}_D{D}_P{P}", "real_sizes", shapes, px, D, 140 + i, aw=aw))
    return cases


FAMILIES = {"lattice": lattice, "border_bands": border_bands, "degenerate_maps": degenerate_maps, "head_dims": head_dims,
            "contention": contention, "weights": weights, "real_sizes": real_sizes}
RANDOM_FAMILIES = ("border_bands", "degenerate_maps", "head_dims", "weights", "real_sizes")
