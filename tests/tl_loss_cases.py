"""Tube-Link's point-sampled training loss (axial_vs_amd.tube_link_losses / axvs_tl_loss_*): a float64 restatement of the whole chain
in plain torch, the case list, the screens and the fixture readers shared by tests/test_tl_loss_cpu.py, tests/test_hip_tl_loss.py and
tools/gen_golden_tl_loss.py.

RESTATEMENT (float64 on the CPU; written from MaXTron_Tube-Link/models/video/tube_link_vis/mask2former_video_cc_head.py:519-694,
mmdet/core/bbox/match_costs/match_cost.py:153-359, core/bbox/assigners/mask_hungarian_assigner.py:113-123,
models/utils/point_sample.py:32-87, models/losses/cross_entropy_loss.py, dice_loss.py and utils.py).  point_sample(img, p) is
F.grid_sample(img, 2 p - 1, 'bilinear', 'zeros', align_corners=False); the long image of a query or of a target is its T frames stacked
along the rows.  Per layer l and video b, with x [Q, P] and g [M, P] sampled at the P shared points match[l, b]:
    cost = -w_c softmax(cls)[:, labels] + w_m (softplus(-x) g^T + softplus(x) (1 - g)^T) / P
           + w_d (1 - (2 sigmoid(x) g^T + eps) / (sum_p sigmoid(x) + sum_p g + eps))
    rows, cols = scipy.optimize.linear_sum_assignment(cost)
Per layer, over its G matched pairs in (video, query) order: |logit| at the S candidates cand[l, g], the k smallest kept (EQUAL values:
the lower index, a stable sort), the P - k points rand[l, g] appended, x and t sampled there;
    loss_cls  = lw_c sum_i w[y_i] CE_i / (sum_i w[y_i] + eps32), y = the matched label, K for an unmatched query
    loss_mask = lw_m sum BCE_with_logits(x, t) / (ntm P + eps32);   loss_dice = lw_d sum_g (1 - (2 sum s t + eps) / (sum s + sum t + eps)) / (ntm + eps32)
with ntm = max(G, 1) and eps32 = 2^-23 (weight_reduce_loss); a layer without a pair has loss_mask = loss_dice = 0.  Gradients come from
autograd on this.

ERROR MEASURES.  A loss scalar: |got - ref| / |ref|.  A cost matrix or a gradient tensor: max|got - ref| / max|ref|.

THE YARDSTICK of the GPU test is the reference's own fp32 CPU result (the fixture) against this restatement, per case and per
quantity -- cost, losses, d cls_scores, d mask_preds --, floored at 2^-24 (one rounding of an fp32 result): the device may be 8 times as far.

SCREENS.  A case is used only at a seed where (1) every assignment is stable: `matcher_cases.stable`, perturbed float64 costs give the
same pairs; (2) for every matched pair with 0 < k < S the gap between the k-th and (k+1)-th smallest |logit| exceeds 8 times the
reference's own fp32 error on those two values (fp32 grid_sample against float64), so the kept SET is the same in every precision.
`find_seed` walks up from the case's first seed; the seeds that pass are fixed in tests/golden/g22_tl_loss_seeds.json and
tests/test_tl_loss_cpu.py asserts the screens at them.

CASES are the smallest shapes at which each part can go wrong:
    Q5_M3         one 32-block with 27 empty rows; T = 1; P = 64 = two tiles; (3, 0.75)
    Q5_M7_k0      M > Q: solved on the transpose, Q pairs; fp32 targets; T = 2 (one frame boundary); (3, 0): k = 0, every point random
    Q5_M5-0_L3    M_b = Q; B = 2 with an empty SECOND video; L = 3; T = 3 (two boundaries); targets at 4 x the resolution; P = 112 (3.5
                  tiles); (1.5, 0.5)
    Q33_M3-1_kS   Q one past a 32-block (two query blocks); B = 2, M = (3, 1); 12 x 20; (1, 1): k = S = P, nothing random
    Q33_M0        no object at all: the zero-match layer
    Q33_M0-3      the FIRST video is empty (its offset into the concatenated targets is the next video's)
    Q100_M3_L3    Q = 100 (four query blocks, the last with 4 rows); L = 3; fp32 targets at 4 x the resolution
    Q100_M8_big   num_points = 12544 once: T = 2, 32 x 57; S = 37632, k = 9408
    saturated     every logit of the matched masks beyond +-30: softplus and sigmoid saturate
    hand_placed   coordinates 0.0, the largest float below 1.0, pixel centres and the frame boundary of the long image (C-ABI case of the
                  GPU test; k = 0 so that match_coords and rand_coords carry them)"""
import hashlib
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

import matcher_cases as mc

GOLDEN = mc.GOLDEN
U32 = mc.U32
FLOOR = 2.0 ** -24
EPS32 = float(torch.finfo(torch.float32).eps)
SEEDS_FILE = os.path.join(GOLDEN, "g22_tl_loss_seeds.json")
COST_W = (2.0, 5.0, 5.0)
LOSS_W = (2.0, 5.0, 5.0)
DICE_EPS = 1.0

#            L  B  Q    K   M        T  h   w   gs kind   P      over ratio  seed0
CASES = {
    "Q5_M3":        dict(L=1, Q=5, K=4, M=(3,), T=1, h=7, w=9, gs=1, kind="u8", P=64, over=3.0, ratio=0.75, seed0=100),
    "Q5_M7_k0":     dict(L=1, Q=5, K=6, M=(7,), T=2, h=7, w=9, gs=1, kind="f32", P=64, over=3.0, ratio=0.0, seed0=200),
    "Q5_M5-0_L3":   dict(L=3, Q=5, K=4, M=(5, 0), T=3, h=7, w=9, gs=4, kind="u8", P=112, over=1.5, ratio=0.5, seed0=300),
    "Q33_M3-1_kS":  dict(L=1, Q=33, K=7, M=(3, 1), T=2, h=12, w=20, gs=1, kind="u8", P=112, over=1.0, ratio=1.0, seed0=400),
    "Q33_M0":       dict(L=1, Q=33, K=7, M=(0,), T=1, h=12, w=20, gs=1, kind="u8", P=64, over=3.0, ratio=0.75, seed0=500),
    "Q33_M0-3":     dict(L=1, Q=33, K=7, M=(0, 3), T=3, h=12, w=20, gs=1, kind="f32", P=64, over=3.0, ratio=0.75, seed0=600),
    "Q100_M3_L3":   dict(L=3, Q=100, K=10, M=(3,), T=1, h=7, w=9, gs=4, kind="f32", P=64, over=3.0, ratio=0.75, seed0=700),
    "Q100_M8_big":  dict(L=1, Q=100, K=10, M=(8,), T=2, h=32, w=57, gs=1, kind="u8", P=12544, over=3.0, ratio=0.75, seed0=800),
    "saturated":    dict(L=1, Q=5, K=4, M=(3,), T=2, h=7, w=9, gs=1, kind="u8", P=64, over=3.0, ratio=0.75, seed0=900, saturate=True),
    "hand_placed":  dict(L=1, Q=5, K=4, M=(3,), T=2, h=7, w=9, gs=1, kind="u8", P=64, over=1.0, ratio=0.0, seed0=1000, hand=True),
}
BIG = ("Q100_M8_big",)
DMASK_STRIDE = 61          # the big case stores every 61st element of d mask_preds


def counts(c):
    """(S, k, G)"""
    return int(c["P"] * c["over"]), int(c["ratio"] * c["P"]), sum(min(c["Q"], m) for m in c["M"])


def upstream_weights(L):
    return [1.0 + 0.25 * np.sin(1.0 + i) for i in range(3 * L)]


def loss_keys(L):
    names = ("loss_cls", "loss_mask", "loss_dice")
    return list(names) + [f"d{i}.{n}" for i in range(L - 1) for n in names]


def layer_of_key(L):
    """position of every dict key in the [L, 3] loss array, in `loss_keys` order"""
    return [3 * (L - 1) + j for j in range(3)] + [3 * i + j for i in range(L - 1) for j in range(3)]


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def make_inputs(c, seed):
    """cls_scores [L][B, Q, K + 1], mask_preds [L][B, T, Q, h, w] (fp32), labels [B][M_b] int64, masks [B][M_b, T, Hg, Wg] (uint8 or fp32),
    class_weight.  Object m of a video is a box that drifts over the frames; query perm[m] of every layer predicts it (logits +-2.5 plus
    noise), so the assignment has a clear optimum, and the other queries are noise."""
    g = torch.Generator().manual_seed(seed)
    L, Q, K, T, h, w, gs = c["L"], c["Q"], c["K"], c["T"], c["h"], c["w"], c["gs"]
    B, Hg, Wg = len(c["M"]), h * gs, w * gs
    labels, masks, coarse = [], [], []
    for M in c["M"]:
        labels.append(torch.randint(0, K, (M,), generator=g))
        t = torch.zeros(M, T, Hg, Wg)
        for m in range(M):
            y0, x0 = int(torch.randint(0, Hg // 2, (1,), generator=g)), int(torch.randint(0, Wg // 2, (1,), generator=g))
            hh, ww = int(torch.randint(Hg // 4 + 1, Hg // 2 + 1, (1,), generator=g)), int(torch.randint(Wg // 4 + 1, Wg // 2 + 1, (1,), generator=g))
            for f in range(T):
                t[m, f, min(y0 + f * gs, Hg - 1):y0 + f * gs + hh, x0:x0 + ww] = 1.0
        if c["kind"] == "f32":
            t = t * (0.25 + 0.75 * torch.rand(M, T, Hg, Wg, generator=g))
            masks.append(t)
        else:
            masks.append(t.to(torch.uint8))
        coarse.append(F.adaptive_avg_pool2d(t.reshape(M * T, 1, Hg, Wg), (h, w)).reshape(M, T, h, w) if M else t.reshape(0, T, h, w))
    cls, preds = [], []
    amp = 40.0 if c.get("saturate") else 2.5
    for _ in range(L):
        cl = torch.randn(B, Q, K + 1, generator=g)
        pm = torch.randn(B, T, Q, h, w, generator=g) * (0.0 if c.get("saturate") else 1.0)
        if c.get("saturate"):
            pm = pm - 35.0
        for b, M in enumerate(c["M"]):
            perm = torch.randperm(Q, generator=g)
            for m in range(min(M, Q)):
                q = int(perm[m])
                pm[b, :, q] = (2.0 * coarse[b][m] - 1.0) * amp + 0.5 * torch.randn(T, h, w, generator=g)
                cl[b, q, labels[b][m]] += 2.0
        cls.append(cl)
        preds.append(pm)
    cw = torch.tensor([1.0] * K + [0.1])
    return dict(cls=cls, masks=preds, labels=labels, gt=masks, class_weight=cw)


def draw(c, seed, device="cpu", draw_point_coords=None):
    """the case's coordinates: axial_vs_amd.draw_point_coords under the case's seed (+ 1: the inputs took `seed`)"""
    if draw_point_coords is None:
        from axial_vs_amd.tl_criterion import draw_point_coords
    gen = torch.Generator(device=device).manual_seed(seed + 1)
    coords = draw_point_coords(c["L"], c["M"], c["Q"], c["P"], c["over"], c["ratio"], device, generator=gen)
    if c.get("hand"):
        coords = hand_place(c, coords)
    return coords


def hand_place(c, coords):
    """overwrite the first points of match_coords and rand_coords: 0.0, the largest float below 1.0, pixel centres (also the first and
    last pixel), and points on and next to the frame boundary of the long image (row T*h / 2 for T = 2: y = 0.5)"""
    match, cand, rand = [t.clone() for t in coords]
    one = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
    R, w = c["T"] * c["h"], c["w"]
    pts = [(0.0, 0.0), (one, one), (0.0, one), (one, 0.0),
           (0.5 / w, 0.5 / R), ((w - 0.5) / w, (R - 0.5) / R), (3.5 / w, 4.5 / R), (4.5 / w, (c["h"] - 0.5) / R), (4.5 / w, (c["h"] + 0.5) / R),
           (0.3, 0.5), (0.7, c["h"] / R), (2.5 / w, 0.5 - 0.2 / R), (2.5 / w, 0.5 + 0.2 / R), (one, 0.5), (0.0, 0.5)]
    v = torch.tensor(pts, dtype=torch.float32)
    match[:, :, :len(pts)] = v
    rand[:, :, :len(pts)] = v
    return match, cand, rand


# ---- the restatement --------------------------------------------------------------------------------------------------------------------
def point_sample(img, pts):
    """img [N, R, W], pts [N, P, 2] in [0, 1) -> [N, P]"""
    return F.grid_sample(img[:, None], 2.0 * pts[:, :, None, :] - 1.0, mode="bilinear", padding_mode="zeros", align_corners=False)[:, 0, :, 0]


def long_pred(mp):
    """mask_preds of a video [T, Q, h, w] -> [Q, T*h, w]"""
    return mp.transpose(0, 1).flatten(1, 2)


def cost_of(cls, x, g, labels, dt):
    P = x.shape[1]
    c_cls = -cls.softmax(-1)[:, labels]
    c_mask = (F.softplus(-x) @ g.T + F.softplus(x) @ (1.0 - g).T) / P
    s = x.sigmoid()
    c_dice = 1.0 - (2.0 * (s @ g.T) + DICE_EPS) / (s.sum(-1)[:, None] + g.sum(-1)[None, :] + DICE_EPS)
    return COST_W[0] * c_cls + COST_W[1] * c_mask + COST_W[2] * c_dice


def restate(c, inp, coords, dt=torch.float64, weights=None, pairs=None, selected=None):
    """-> dict(cost [L][B] (None for an empty video), rows / cols [L][B], selected [L] (int64 [G, k], increasing), keys [L] ([G, S] |logit|),
    losses [L, 3], dcls [L], dmasks [L]).  `pairs` / `selected` given: used instead of the restatement's own (for a precision other than float64)."""
    from scipy.optimize import linear_sum_assignment
    L, Q, K, P = c["L"], c["Q"], c["K"], c["P"]
    S, k, G = counts(c)
    match, cand, rand = [t.to(dt) for t in coords]
    cls = [t.to(dt).requires_grad_(True) for t in inp["cls"]]
    mps = [t.to(dt).requires_grad_(True) for t in inp["masks"]]
    cw = inp["class_weight"].to(dt)
    out = dict(cost=[], rows=[], cols=[], selected=[], keys=[])
    losses = []
    for l in range(L):
        costs, rows, cols, labs, px, tg = [], [], [], [], [], []
        for b, M in enumerate(c["M"]):
            lab = torch.full((Q,), K, dtype=torch.int64)
            if M == 0:
                costs.append(None); rows.append(torch.zeros(0, dtype=torch.int64)); cols.append(torch.zeros(0, dtype=torch.int64)); labs.append(lab)
                continue
            with torch.no_grad():
                lp = long_pred(mps[l][b])
                x = point_sample(lp, match[l, b][None].expand(Q, -1, -1))
                gl = inp["gt"][b].to(dt).flatten(1, 2)
                g = point_sample(gl, match[l, b][None].expand(M, -1, -1))
                C = cost_of(cls[l][b], x, g, inp["labels"][b], dt)
            if pairs is None:
                r, cc = linear_sum_assignment(C.numpy())
                r, cc = torch.as_tensor(r, dtype=torch.int64), torch.as_tensor(cc, dtype=torch.int64)
            else:
                r, cc = pairs[l][b]
            lab[r] = inp["labels"][b][cc]
            costs.append(C); rows.append(r); cols.append(cc); labs.append(lab)
            px.append(long_pred(mps[l][b])[r])
            tg.append(inp["gt"][b].to(dt).flatten(1, 2)[cc])
        out["cost"].append(costs); out["rows"].append(rows); out["cols"].append(cols)
        lab = torch.cat(labs)
        ce = F.cross_entropy(cls[l].flatten(0, 1), lab, weight=cw, reduction="none")
        loss_cls = LOSS_W[0] * ce.sum() / (cw[lab].sum() + EPS32)
        if G == 0:
            zero = torch.zeros((), dtype=dt)
            losses.append(torch.stack([loss_cls, zero, zero]))
            out["selected"].append(torch.zeros(0, k, dtype=torch.int64)); out["keys"].append(torch.zeros(0, S, dtype=dt))
            continue
        px, tg = torch.cat(px), torch.cat(tg)
        with torch.no_grad():
            keys = point_sample(px, cand[l]).abs() if S > 0 else torch.zeros(G, 0, dtype=dt)
            if selected is None:
                idx = torch.from_numpy(np.sort(np.argsort(keys.numpy(), axis=1, kind="stable")[:, :k], axis=1)).long()
            else:
                idx = selected[l]
            pts = torch.cat([torch.gather(cand[l], 1, idx[:, :, None].expand(-1, -1, 2)), rand[l]], 1)
            t = point_sample(tg, pts)
        out["selected"].append(idx); out["keys"].append(keys)
        x = point_sample(px, pts)
        ntm = max(float(G), 1.0)
        loss_mask = LOSS_W[1] * F.binary_cross_entropy_with_logits(x, t, reduction="none").sum() / (ntm * P + EPS32)
        s = x.sigmoid()
        dice = 1.0 - (2.0 * (s * t).sum(1) + DICE_EPS) / (s.sum(1) + t.sum(1) + DICE_EPS)
        loss_dice = LOSS_W[2] * dice.sum() / (ntm + EPS32)
        losses.append(torch.stack([loss_cls, loss_mask, loss_dice]))
    losses = torch.stack(losses)
    w = torch.tensor(upstream_weights(L) if weights is None else weights, dtype=dt)
    (losses.reshape(-1) * w).sum().backward()
    out["losses"] = losses.detach()
    out["dcls"] = [t.grad if t.grad is not None else torch.zeros_like(t) for t in cls]
    out["dmasks"] = [t.grad if t.grad is not None else torch.zeros_like(t) for t in mps]
    return out


# ---- screens ----------------------------------------------------------------------------------------------------------------------------
def screens(c, inp, coords, r64=None):
    """(assignments stable, selection gaps wide enough, smallest gap / (8 x fp32 error) over the pairs)"""
    r64 = restate(c, inp, coords) if r64 is None else r64
    S, k, G = counts(c)
    ok_assign = all(C is None or mc.stable(C, r, cc, trials=50) for Cs, rs, cs in zip(r64["cost"], r64["rows"], r64["cols"])
                    for C, r, cc in zip(Cs, rs, cs))
    worst = float("inf")
    if G > 0 and 0 < k < S:
        for l in range(c["L"]):
            px = torch.cat([long_pred(inp["masks"][l][b])[r64["rows"][l][b]] for b in range(len(c["M"])) if c["M"][b] > 0])
            keys = r64["keys"][l]
            order = torch.from_numpy(np.argsort(keys.numpy(), axis=1, kind="stable"))
            two = order[:, k - 1:k + 1]                                              # the k-th and (k+1)-th smallest
            pts = torch.gather(coords[1][l], 1, two[:, :, None].expand(-1, -1, 2))
            x32 = point_sample(px.float(), pts.float()).abs().double()                # the reference's own fp32 values
            x64 = torch.gather(keys, 1, two)
            err = (x32 - x64).abs().max(1).values
            gap = x64[:, 1] - x64[:, 0]
            ratio = torch.where(err > 0, gap / (8.0 * err), torch.where(gap > 0, torch.full_like(gap, float("inf")), torch.zeros_like(gap)))
            worst = min(worst, float(ratio.min()))
    return ok_assign, worst > 1.0, worst


def find_seed(c, tries=50):
    for seed in range(c["seed0"], c["seed0"] + tries):
        inp = make_inputs(c, seed)
        a, s, _ = screens(c, inp, draw(c, seed))
        if a and s:
            return seed
    raise RuntimeError("no seed passes the screens")


def seeds():
    with open(SEEDS_FILE) as f:
        return json.load(f)


# ---- error measures ---------------------------------------------------------------------------------------------------------------------
def scalar_err(got, ref):
    got, ref = float(got), float(ref)
    if ref == 0.0:
        return 0.0 if got == 0.0 else float("inf")
    return abs(got - ref) / abs(ref)


def tensor_err(got, ref):
    got, ref = got.double().cpu(), ref.double().cpu()
    if ref.numel() == 0:
        return 0.0
    scale = float(ref.abs().max())
    if scale == 0.0:
        return 0.0 if float(got.abs().max()) == 0.0 else float("inf")
    return float((got - ref).abs().max()) / scale


def digest(t):
    return hashlib.sha256(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes()).hexdigest()


# ---- fixtures -----------------------------------------------------------------------------------------------------------------------------
class Fixture:
    """one case at its fixed seed: regenerated inputs and coordinates, the reference's stored fp32 results, the float64 restatement
    (computed once, shared)"""

    def __init__(self, name):
        self.name, self.c = name, CASES[name]
        self.seed = seeds()[name]
        z = np.load(os.path.join(GOLDEN, f"g22_tl_loss_{name}.npz"))
        self.meta = json.loads(bytes(z["meta"]).decode())
        c, L, B = self.c, self.c["L"], len(self.c["M"])
        self.inp = make_inputs(c, self.seed)
        self.coords = draw(c, self.seed)
        self.ref_pairs = [[(torch.from_numpy(z[f"rows_{l}_{b}"]).long(), torch.from_numpy(z[f"cols_{l}_{b}"]).long()) for b in range(B)] for l in range(L)]
        self.ref_cost = [[torch.from_numpy(z[f"cost_{l}_{b}"]) if c["M"][b] > 0 else None for b in range(B)] for l in range(L)]
        self.ref_selected = [torch.from_numpy(z[f"sel_{l}"].astype(np.int64)) for l in range(L)] if "sel_0" in z else None
        self.ref_losses = torch.from_numpy(z["ref_losses"])
        self.ref_dcls = [torch.from_numpy(z[f"ref_dcls_{l}"]) for l in range(L)]
        self.ref_dmasks = [torch.from_numpy(z[f"ref_dmasks_{l}"]) for l in range(L)]          # the big case: every DMASK_STRIDE-th element
        self._r64 = None

    def restated(self):
        if self._r64 is None:
            self._r64 = restate(self.c, self.inp, self.coords)
        return self._r64

    def sub(self, dmask):
        return dmask.reshape(-1)[::DMASK_STRIDE] if self.name in BIG else dmask

    def yard(self):
        """the reference's own fp32 errors against the restatement, floored: dict(cost, losses, dcls, dmasks)"""
        r = self.restated()
        L, B = self.c["L"], len(self.c["M"])
        ec = max([tensor_err(self.ref_cost[l][b], r["cost"][l][b]) for l in range(L) for b in range(B) if self.c["M"][b] > 0] or [0.0])
        el = max(scalar_err(self.ref_losses[l, j], r["losses"][l, j]) for l in range(L) for j in range(3))
        egc = max(tensor_err(self.ref_dcls[l], r["dcls"][l]) for l in range(L))
        egm = max(tensor_err(self.ref_dmasks[l], self.sub(r["dmasks"][l])) for l in range(L))
        return dict(cost=max(ec, FLOOR), losses=max(el, FLOOR), dcls=max(egc, FLOOR), dmasks=max(egm, FLOOR))


_cache = {}


def fixture(name):
    if name not in _cache:
        _cache[name] = Fixture(name)
    return _cache[name]
