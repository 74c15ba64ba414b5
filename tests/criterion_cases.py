"""The set criterion (axial_vs_amd.MaXTronCCSetCriterion / set_criterion_losses): a float64 restatement of the reference's `labels` and
`masks` losses (MaXTron_Video-kMaX/maxtron_deeplab/modeling/cc_criterion.py:144-200, :237-266, :338-412) in plain torch, the fixture
readers and the error measures shared by tests/test_criterion_cpu.py, tests/test_hip_criterion.py and tools/gen_golden_criterion.py.

RESTATEMENT (all float64, on the fixture's stored input values; layer 0 is the final prediction, layer 1 + i is aux_outputs[i]).  Per
layer and video, with (rows, cols) the matched pairs, x = pred_masks [N, P], P = T*H*W:
    t[rows]     = masks[cols], 0 elsewhere;   void[p] = sum_n t[n, p] < 1;   keep = ~void iff masking_void_pixel else all
    w_mask[rows] = clamp(class similarity at the pairs, 1e-5), 0 elsewhere
    w_cls       = sum_p prob void / (sum_p prob + 1e-5) with prob = softmax_n(x);  w_cls[rows] = mask similarity at the pairs;  clamp 1e-5
    label[rows] = labels[cols], num_classes elsewhere
    loss_mask   = mean_b sum_p ce / max(#{ce != 0}, 1),   ce = keep * -sum_n t log_softmax_n(x)
    loss_dice   = mean_b sum_n (1 - (2 sum_p keep prob t + 1) / (sum_p keep prob + sum_p t + 1)) w_mask * 0.75 / N
    loss_ce     = mean_b sum_n a_n w_cls CE(pred_logits[n], label[n]) / max(#nonzero, 1),   a = 0.75 (0.25 for the void class)
With share_final_matching the pairs, t, void and both weights of layer 0 serve every layer (the void IoU is taken on layer 0's masks);
otherwise each layer has its own.  The similarities at the pairs are the matcher restatement's (tests/matcher_cases.py), in float64 too.
Gradients come from autograd on this.

ERROR MEASURES.  A loss scalar: |got - ref| / |ref|.  A gradient tensor: max|got - ref| / max|ref|.

THE YARDSTICK of the GPU test is the reference's own fp32 CPU result against this restatement, per fixture, taken separately over the
3 L loss scalars and over the 2 L gradient tensors, floored at 2^-24 (one rounding of an fp32 result): the device may be 8 times as far
from float64.  The margin covers another summation order over P and different exp / division roundings; it is not fitted to the kernels.

THE BOUND of the CPU test on the reference's fp32 values is derived from the number format (u = 2^-24), as in matcher_cases: a softmax
or log-softmax value carries (N + 4) u, a sum of P non-negative terms at most (P - 1) u more whatever the order, a ratio of two such sums
twice that plus the division, and each loss is a product / mean of a few such ratios and of the matcher's similarities
(fp32_bound_mask): fp32_bound = 4 (P + N + K + 8) u.  The same bound, relative to the largest entry, holds for a gradient element, which is
a short sum of products of such quantities.

EDGE CASES.  CASES sits on the grid the kernels were written for: N a multiple of 4 (wave g of a workgroup holds the queries g, g + 4, ...)
and P of 1 to 4 tiles of 64 pixels or an even split.  EDGE_CASES are fixtures of the same kind at the sizes where the guard code runs;
a problem gets min(ceil(512 / (L B)), ceil(ntiles / 4)) workgroups of ceil(ntiles / that) tiles, the last one with what is left.
    N = 1, P = 1, K + 1 = 2   three waves without a query, every ce exactly 0 (count = max(0, 1)), d pred_masks zero in exact arithmetic
    N = 2, M = (1, 3)         N < 4; M = 3 > N is solved on the transpose; own matching per layer; P = 65: one full tile and one pixel
    N = 3, M = (2, 0)         N < 4; P = 63: a single partial tile; the second video has no object; shared matching over 3 layers; float
    N = 5, M = (0, 4)         wave 0 holds two queries, the others one; the FIRST video has no object (its offset into the concatenated
                              targets is the next video's); P = 300: 5 tiles, two workgroups of 3 and 2 tiles (the second one's range is
                              clamped, starts on an odd tile and ends on a 44-pixel tile); 5 tiles split evenly under no plan of >= 2 tiles
    N = 7, M = (9, 2)         waves of 2, 2, 2 and 1 queries; M = 9 > N; no masking; the same split; the case of the input-form tests
    N = 127                   the top register slot of wave 3 is empty (the unrolled `q < N` guard at 32 slots); the same split
    N = 129, M = (4, 3)       the first N of the any-size kernels, wave 0's last query alone; two videos with their own matching per layer;
                              the any-size kernels on two workgroups
    N = 130, P = 581          10 tiles: three workgroups of 4, 4 and 2 tiles on the any-size kernels; float targets
    N = 260, M = 40           the any-size kernels' LDS arrays beyond 256; in the matcher 9 x 2 = 18 output blocks, so two block chunks,
                              on two pixel workgroups, with more than 48 KB of dynamic LDS
    N = 512, P = 70           the bound on N
    N = 6, M = (0, 0)         no video has an object: mask and dice losses exactly 0, the class loss comes from the void IoU alone
UNSCREENED_CASES holds what the reference cannot give a screened fixture for: objects whose masks are all zero (target kind "blank";
N = 6, P = 65).  Every similarity is 0, every assignment ties, and the stability screen fails by construction.  Under masking every
pixel is void; the tests assert the exact zeros and compare the class loss with the restatement on the device's own pairs."""
import json
import os

import numpy as np
import torch

import matcher_cases as mc

GOLDEN = mc.GOLDEN
U32 = mc.U32
FLOOR = 2.0 ** -24

# name: (N, objects per video, K, T, H, W, layers, share_final_matching, masking_void_pixel, target kind)
CASES = {
    "g19_criterion_N16_M5-0_L3_share_mv1": (16, (5, 0), 7, 2, 6, 10, 3, 1, 1, "bool"),
    "g19_criterion_N16_M5-0_L3_share_mv0": (16, (5, 0), 7, 2, 6, 10, 3, 1, 0, "bool"),
    "g19_criterion_N20_M33-7_L3_own_mv1": (20, (33, 7), 10, 2, 9, 13, 3, 0, 1, "bool"),
    "g19_criterion_N20_M7-3_L2_own_mv1_float": (20, (7, 3), 10, 2, 9, 13, 2, 0, 1, "float"),
    "g19_criterion_N20_M7-3_L2_share_mv0_float": (20, (7, 3), 10, 2, 9, 13, 2, 1, 0, "float"),
    "g19_criterion_N128_M23_L2_share_mv1": (128, (23,), 124, 4, 16, 16, 2, 1, 1, "bool"),
    "g19_criterion_N100_M1_L1_share_mv1": (100, (1,), 40, 1, 8, 8, 1, 1, 1, "bool"),
}
BIG, RAGGED = "g19_criterion_N128_M23_L2_share_mv1", "g19_criterion_N20_M33-7_L3_own_mv1"

# The edges of the kernels' guard code, in the same format (see EDGE CASES above)
EDGE_CASES = {
    "g19_criterion_N1_M1_L1_share_mv1": (1, (1,), 1, 1, 1, 1, 1, 1, 1, "bool"),
    "g19_criterion_N2_M1-3_L2_own_mv1": (2, (1, 3), 3, 1, 5, 13, 2, 0, 1, "bool"),
    "g19_criterion_N3_M2-0_L3_share_mv1_float": (3, (2, 0), 4, 1, 7, 9, 3, 1, 1, "float"),
    "g19_criterion_N5_M0-4_L2_own_mv1": (5, (0, 4), 6, 1, 4, 75, 2, 0, 1, "bool"),
    "g19_criterion_N7_M9-2_L2_share_mv0": (7, (9, 2), 5, 2, 5, 30, 2, 1, 0, "bool"),
    "g19_criterion_N127_M6_L1_share_mv1": (127, (6,), 9, 1, 5, 60, 1, 1, 1, "bool"),
    "g19_criterion_N129_M4-3_L2_own_mv1": (129, (4, 3), 9, 1, 4, 75, 2, 0, 1, "bool"),
    "g19_criterion_N130_M5_L1_share_mv1_float": (130, (5,), 3, 1, 7, 83, 1, 1, 1, "float"),
    "g19_criterion_N260_M40_L1_share_mv1": (260, (40,), 10, 1, 4, 75, 1, 1, 1, "bool"),
    "g19_criterion_N512_M3_L1_share_mv1": (512, (3,), 5, 1, 2, 35, 1, 1, 1, "bool"),
    "g19_criterion_N6_M0-0_L2_share_mv1": (6, (0, 0), 4, 1, 5, 13, 2, 1, 1, "bool"),
}
# the edge cases whose pixel range is split over workgroups (the GPU test asserts the split from the library's size query), and the two
# of them that run the any-size kernels
SPLIT = ["g19_criterion_N5_M0-4_L2_own_mv1", "g19_criterion_N7_M9-2_L2_share_mv0", "g19_criterion_N127_M6_L1_share_mv1",
         "g19_criterion_N129_M4-3_L2_own_mv1", "g19_criterion_N130_M5_L1_share_mv1_float", "g19_criterion_N260_M40_L1_share_mv1"]
ANY_SPLIT = ["g19_criterion_N129_M4-3_L2_own_mv1", "g19_criterion_N130_M5_L1_share_mv1_float"]
# No fixture: every similarity of all-zero targets is 0, every assignment ties, and no matching passes the generator's stability screen
UNSCREENED_CASES = {
    "blank_N6_M3-2_L2_share_mv1": (6, (3, 2), 4, 1, 5, 13, 2, 1, 1, "blank"),
}
KEYS = ("loss_ce", "loss_mask", "loss_dice")


def loss_keys(L):
    """the reference's result keys in its order"""
    return [k if l == 0 else f"{k}_{l - 1}" for l in range(L) for k in KEYS]


def upstream_weights(L):
    """unequal weights of the 3 L scalars, in key order"""
    return [1.0 + 0.1 * i for i in range(3 * L)]


def make_case(case, seed):
    """inputs of a case: layers [{pred_masks [B, N, T, H, W], pred_logits [B, N, K + 1]}] (fp16-representable fp32) and targets"""
    N, Ms, K, T, H, W, L, share, mv, kind = case
    targets = []
    for b, M in enumerate(Ms):
        _, _, labels, tbool, tf = mc.make_inputs(N, M, K, T, H, W, 19500 + 10 * seed + b)
        masks = {"bool": tbool, "float": tf.float(), "blank": torch.zeros_like(tbool)}[kind]       # blank: objects whose masks are all zero
        targets.append({"labels": labels, "masks": masks})
    layers = []
    for l in range(L):
        ins = [mc.make_inputs(N, 1, K, T, H, W, 19600 + 100 * seed + 10 * l + b)[:2] for b in range(len(Ms))]
        layers.append({"pred_masks": torch.stack([p for p, _ in ins]).float(), "pred_logits": torch.stack([x for _, x in ins]).float()})
    return layers, targets


# ---- float64 restatement ------------------------------------------------------------------------------------------------------------
def _processed(src_masks, logits_m, masks_m, tgt, rows, cols, K, matcher_masking):
    """one video's padded targets and weights (constants): t [N, P], void [P], w_mask, w_cls, label [N]"""
    N = src_masks.shape[0]
    x = src_masks.detach().double().flatten(1)
    tm = tgt["masks"].double().flatten(1)
    t = torch.zeros_like(x)
    t[rows] = tm[cols]
    void = t.sum(0) < 1
    w_mask = torch.zeros(N, dtype=torch.float64)
    prob = torch.softmax(x, 0)
    w_cls = (prob * void.double()).sum(-1) / (prob.sum(-1) + 1e-5)
    label = torch.full((N,), K, dtype=torch.int64)
    if rows.numel():
        ms = mc.mask_similarity64(masks_m.detach(), tgt["masks"], matcher_masking)
        cs = mc.class_similarity64(logits_m.detach(), tgt["labels"])
        w_mask[rows] = cs[rows, cols].clamp(min=1e-5)
        w_cls[rows] = ms[rows, cols]
        label[rows] = tgt["labels"][cols]
    return t, void, w_mask, w_cls.clamp(min=1e-5), label


def criterion64(layers, targets, pairs, K, masking, share, matched=None, matcher_masking=None):
    """-> losses float64 [L, 3].  layers: float64 tensors (leaves for autograd); pairs[j][b] = (rows, cols) of matching j (one
    matching when shared, else one per layer); `matched`: the prediction matching 0 was made on (default: layer 0)."""
    L, B = len(layers), len(targets)
    mm = masking if matcher_masking is None else matcher_masking
    out = []
    for l in range(L):
        j = 0 if share else l
        src = layers[j]                                   # process_gt's `outputs`
        mo = matched if (matched is not None and j == 0) else layers[j]      # the matcher's `outputs`
        ce_l, mask_l, dice_l = 0.0, 0.0, 0.0
        for b in range(B):
            rows, cols = pairs[j][b]
            t, void, w_mask, w_cls, label = _processed(src["pred_masks"][b], mo["pred_logits"][b], mo["pred_masks"][b], targets[b], rows, cols, K, mm)
            x = layers[l]["pred_masks"][b].flatten(1)
            N = x.shape[0]
            keep = (~void).double() if masking else torch.ones_like(void, dtype=torch.float64)
            ce = -(t * torch.log_softmax(x, 0)).sum(0) * keep
            mask_l = mask_l + ce.sum() / max(int((ce != 0).sum()), 1)
            q = torch.softmax(x, 0) * keep
            dl = (1.0 - (2.0 * (q * t).sum(-1) + 1.0) / (q.sum(-1) + t.sum(-1) + 1.0)) * w_mask
            dice_l = dice_l + dl.sum() * 0.75 / N
            lg = layers[l]["pred_logits"][b]
            cl = -torch.log_softmax(lg, -1)[torch.arange(N), label]
            f = torch.where(label == K, 0.25, 0.75) * cl * w_cls
            ce_l = ce_l + f.sum() / max(int((f != 0).sum()), 1)
        out.append(torch.stack([ce_l / B, mask_l / B, dice_l / B]))
    return torch.stack(out)


def nonzero_counts64(layers, targets, pairs, K, masking, share):
    """#{ce != 0} per (layer, video) in float64: the screen of the generator"""
    res = []
    for l in range(len(layers)):
        j = 0 if share else l
        for b in range(len(targets)):
            rows, cols = pairs[j][b]
            t, void, *_ = _processed(layers[j]["pred_masks"][b], layers[j]["pred_logits"][b], layers[j]["pred_masks"][b], targets[b], rows, cols, K, masking)
            ce = -(t * torch.log_softmax(layers[l]["pred_masks"][b].double().flatten(1), 0)).sum(0)
            if masking:
                ce = ce * (~void).double()
            res.append(int((ce != 0).sum()))
    return res


def void_pixels(fx):
    """per matching j and video b: bool [P], the pixels the restatement calls void (no matched target has weight >= 1 there in sum)"""
    res = []
    for j, per_video in enumerate(fx.pairs):
        out = []
        for b, (rows, cols) in enumerate(per_video):
            t = torch.zeros(fx.N, fx.P, dtype=torch.float64)
            t[rows] = fx.targets[b]["masks"].double().flatten(1)[cols]
            out.append(t.sum(0) < 1)
        res.append(out)
    return res


def scalar_err(got, ref):
    got, ref = float(got), float(ref)
    if ref == 0.0:
        return 0.0 if got == 0.0 else float("inf")
    return abs(got - ref) / abs(ref)


def grad_err(got, ref):
    got, ref = got.double().cpu(), ref.double().cpu()
    scale = float(ref.abs().max())
    if scale == 0.0:
        return 0.0 if float(got.abs().max()) == 0.0 else float("inf")
    return float((got - ref).abs().max()) / scale


def fp32_bound(N, P, K):
    return 4.0 * (P + N + K + 8) * U32


# ---- fixtures -------------------------------------------------------------------------------------------------------------------------
class CriterionFixture:
    """inputs of one case, the reference's fp32 losses / gradients / indices, and the float64 restatement (computed once, shared)"""

    def __init__(self, name):
        self.name = name
        z = np.load(os.path.join(GOLDEN, name + ".npz"))
        self.meta = m = json.loads(bytes(z["meta"]).decode())
        self.N, self.K, self.L, self.B = m["N"], m["K"], m["L"], len(m["M"])
        self.P = m["T"] * m["H"] * m["W"]
        self.share, self.masking, self.kind = bool(m["share"]), bool(m["masking"]), m["kind"]
        shp = (m["T"], m["H"], m["W"])
        self.layers = [{"pred_masks": torch.from_numpy(z[f"pred_masks_{l}"]).float(), "pred_logits": torch.from_numpy(z[f"pred_logits_{l}"]).float()}
                       for l in range(self.L)]
        self.targets = []
        for b, mb in enumerate(m["M"]):
            masks = mc.unpack_bool(z[f"tgt_{b}"], (mb,) + shp) if self.kind == "bool" else torch.from_numpy(z[f"tgt_{b}"]).float()
            self.targets.append({"labels": torch.from_numpy(z[f"labels_{b}"]), "masks": masks})
        nm = 1 if self.share else self.L
        self.pairs = [[(torch.from_numpy(z[f"rows_{j}_{b}"]), torch.from_numpy(z[f"cols_{j}_{b}"])) for b in range(self.B)] for j in range(nm)]
        self.ref_losses = torch.from_numpy(z["ref_losses"])                       # fp32 [L, 3]
        self.ref_dlogits = [torch.from_numpy(z[f"ref_dlogits_{l}"]) for l in range(self.L)]
        self.ref_dmasks = [torch.from_numpy(np.load(os.path.join(GOLDEN, f"{name}_dmasks{l}.npz"))["ref_dmasks"]) for l in range(self.L)]
        self._restated = {}

    def outputs(self, device=None, requires_grad=False):
        """the dict a model hands the criterion: the final prediction = layer 0, aux_outputs = the others"""
        ls = []
        for o in self.layers:
            d = {k: (v if device is None else v.to(device)).clone().requires_grad_(requires_grad) for k, v in o.items()}
            ls.append(d)
        return dict(ls[0], aux_outputs=ls[1:]) if self.L > 1 else dict(ls[0])

    def targets_on(self, device):
        return [{k: v.to(device) for k, v in t.items()} for t in self.targets]

    def restated(self, weights=None):
        """(losses float64 [L, 3], d pred_masks per layer, d pred_logits per layer) of sum_i w_i loss_i (w = 1 by default)"""
        key = None if weights is None else tuple(weights)
        if key not in self._restated:
            ls = [{k: v.double().requires_grad_(True) for k, v in o.items()} for o in self.layers]
            losses = criterion64(ls, self.targets, self.pairs, self.K, self.masking, self.share)
            w = torch.ones(3 * self.L, dtype=torch.float64) if weights is None else torch.tensor(weights, dtype=torch.float64)
            (losses.reshape(-1) * w).sum().backward()
            self._restated[key] = (losses.detach(), [o["pred_masks"].grad for o in ls], [o["pred_logits"].grad for o in ls])
        return self._restated[key]

    def reference_errors(self):
        """the reference's own fp32 errors against the restatement: (largest over the 3 L scalars, largest over the 2 L gradient tensors)"""
        losses, dm, dl = self.restated()
        el = max(scalar_err(self.ref_losses[l, k], losses[l, k]) for l in range(self.L) for k in range(3))
        eg = max(max(grad_err(self.ref_dmasks[l], dm[l]), grad_err(self.ref_dlogits[l], dl[l])) for l in range(self.L))
        return el, eg

    def yard(self):
        el, eg = self.reference_errors()
        return max(el, FLOOR), max(eg, FLOOR)


_cache = {}


def fixture(name):
    if name not in _cache:
        _cache[name] = CriterionFixture(name)
    return _cache[name]
