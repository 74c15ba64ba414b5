"""Prediction-to-ground-truth matching (axial_vs_amd.VideoHungarianMatcher): a float64 restatement of the reference's matcher
(MaXTron_Video-kMaX/maxtron_deeplab/modeling/matcher.py:18-45, :76-92), the fixture readers, the input generators and the error
measures shared by tests/test_matcher_cpu.py, tests/test_hip_matcher.py and tools/gen_golden_matcher.py.

RESTATEMENT (all float64, on the fixture's stored input values):
    prob        = softmax over the Q queries of pred_masks [Q, P], P = T*H*W
    nonvoid[p]  = sum_m t[m, p] > 0;  prob *= nonvoid  iff masking_void_pixel
    mask_sim    = (prob @ t^T) / ((prob.sum(-1)[:, None] + t.sum(-1)[None, :]) / 2 + 1e-5)
    class_sim   = softmax(pred_logits, -1)[:, :-1][:, labels]
    C           = -mask_sim * class_sim;  (row_ind, col_ind) = scipy.optimize.linear_sum_assignment(C)

ERROR MEASURE.  rel_err(got, ref64) is the largest |got - ref| / |ref| over the elements with ref != 0; where ref == 0 (a target that
is empty, or void everywhere a query has mass) got must be 0 exactly, otherwise the measure is inf.

THE YARDSTICK of the GPU per-element test is the reference's own fp32 result against this restatement, per fixture and flag
combination (`reference_error`): the device result may be 8 times as far from float64 as the reference's fp32 CPU result is.  The
margin covers another summation order over P and the different exp / division roundings; it is not fitted to the kernels.

THE BOUND of the CPU test on the reference's fp32 values is derived from the number format (u = 2^-24): a softmax value carries
(Q + 4) u (a sum of Q exps, the exp, the division), a sum of P such non-negative terms at most (P - 1) u more whatever the order,
the ratio of two such sums twice that plus the division: fp32_bound_mask = 2 (P + Q + 4) u; the class similarity is one softmax
value: fp32_bound_class = (K + 1 + 4) u; a matched cost is their product."""
import json
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U32 = 2.0 ** -24

# (Q, M, K, T, H, W): the per-element cases.  P = T*H*W is 120, 768, 64, 234, 1024 -- 234 and 120 are no multiple of the 64-pixel tile,
# M = 33 > Q = 20 is solved on the transpose, M = 1 and M = 33 / 23 / 5 are no multiple of the 32-wide MFMA block, Q = 100 / 20 / 16 neither.
# The sixth shape has 9 x 2 = 18 output blocks of 32 x 32: more than the 16 one workgroup holds, so the similarity kernel runs it in two
# block chunks (each chunk repeats the softmax of its pixels).  Every Q here is a multiple of 4 (wave g holds the queries g, g + 4, ...) and
# every P at most 4 tiles or an even split over the pixel workgroups: what that leaves out is EDGE_SHAPES below.
SHAPES = [(16, 5, 7, 2, 6, 10), (128, 23, 124, 2, 16, 24), (100, 1, 40, 1, 8, 8), (20, 33, 10, 2, 9, 13), (128, 64, 124, 4, 16, 16),
          (288, 40, 10, 2, 8, 13)]
# (Q, M, K, T, H, W) without reference fixtures, checked against `restate` at the format-derived bounds: what the grid of SHAPES leaves out.
#   (5, 3, P = 300)    Q = 5: wave 0 holds two queries, the others one.  5 tiles: two workgroups of 3 and 2 tiles, the second with a clamped
#                      range, starting on an odd tile and ending on a 44-pixel one.
#   (3, 40, P = 63)    Q = 3 < 4: a wave without a query.  One partial tile.  M > Q: solved on the transpose; 63 pixels over 40 objects leave
#                      some targets empty (similarity exactly 0).
#   (260, 40, P = 300) 9 x 2 = 18 output blocks, so two block chunks, which here meet two pixel workgroups; 352 LDS rows = 91.5 KB of
#                      dynamic LDS (above the 48 KB a kernel gets without asking).
EDGE_SHAPES = [(5, 3, 6, 1, 4, 75), (3, 40, 4, 1, 7, 9), (260, 40, 10, 1, 4, 75)]
EDGE_SEED = 18500


def edge_inputs(s):
    """(pred, logits, labels, {"bool": , "float": } targets) of an EDGE_SHAPES entry"""
    pred, logits, labels, tbool, tf = make_inputs(*s, EDGE_SEED + s[0])
    return pred.float(), logits, labels, {"bool": tbool, "float": tf.float()}


# (target kind, masking_void_pixel) combinations stored per shape: all four on the shapes with a small cost matrix, the two diagonal ones
# on the others (their outputs are what makes a fixture big)
ALL_COMBOS = [("bool", 1), ("bool", 0), ("float", 1), ("float", 0)]
E2E = ["g18_matcher_e2e_Q16_M5-0_L3", "g18_matcher_e2e_Q20_M33-7_L3"]


def shape_name(s):
    return "g18_matcher_Q%d_M%d_K%d_T%d_H%d_W%d" % tuple(s)


def combos_of(s):
    Q, M, K, T, H, W = s
    return ALL_COMBOS if Q * M <= 1000 else [("bool", 1), ("float", 0)]


# ---- inputs (the generator stores them; values are fp16-representable so that a 16-bit pred_masks run sees the same numbers) ----------
def make_inputs(Q, M, K, T, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    pred = (torch.randn(Q, T, H, W, generator=g) * 3.0).half()
    logits = (torch.randn(Q, K + 1, generator=g) * 2.0).half().float()
    labels = torch.randint(0, K, (M,), generator=g)
    # panoptic-like binary targets: every pixel belongs to one object or to none (void, about 1 in 5)
    owner = torch.randint(0, M + max(1, M // 4), (T, H, W), generator=g)
    tbool = torch.stack([owner == m for m in range(M)]) if M else torch.zeros(0, T, H, W, dtype=torch.bool)
    # non-binary float targets: overlapping soft masks, void where no object has weight
    tf = torch.rand(M, T, H, W, generator=g) * (torch.rand(M, T, H, W, generator=g) < 0.4)
    tf = (tf * (torch.rand(1, T, H, W, generator=g) < 0.8)).half()
    return pred, logits, labels, tbool, tf


# ---- float64 restatement ------------------------------------------------------------------------------------------------------------
def mask_similarity64(pred, tgt, masking):
    p = torch.softmax(pred.double().flatten(1), 0)
    t = tgt.double().flatten(1)
    if masking:
        p = p * (t.sum(0, keepdim=True) > 0).double()
    inter = p @ t.T
    den = (p.sum(-1)[:, None] + t.sum(-1)[None, :]) / 2.0
    return inter / (den + 1e-5)


def class_similarity64(logits, labels):
    return torch.softmax(logits.double(), -1)[:, :-1][:, labels]


def restate(pred, logits, tgt, labels, masking):
    """-> mask_sim, class_sim, C (float64 [Q, M]) and SciPy's (row_ind, col_ind) on C"""
    from scipy.optimize import linear_sum_assignment
    ms = mask_similarity64(pred, tgt, masking)
    cs = class_similarity64(logits, labels)
    C = -ms * cs
    r, c = linear_sum_assignment(C.numpy())
    return ms, cs, C, torch.as_tensor(r, dtype=torch.int64), torch.as_tensor(c, dtype=torch.int64)


def stable(C64, rows, cols, trials=200, eps=1e-6, seed=0):
    """the optimum of C64 is unchanged under `trials` random perturbations of +-eps on every entry"""
    from scipy.optimize import linear_sum_assignment
    rng = np.random.default_rng(seed)
    C = C64.numpy()
    for _ in range(trials):
        r, c = linear_sum_assignment(C + rng.uniform(-eps, eps, C.shape))
        if not (np.array_equal(r, rows.numpy()) and np.array_equal(c, cols.numpy())):
            return False
    return True


def rel_err(got, ref):
    got, ref = got.double().cpu(), ref.double().cpu()
    if ref.numel() == 0:
        return 0.0
    z = ref == 0
    if bool((got[z] != 0).any()):
        return float("inf")
    if bool(z.all()):
        return 0.0
    return float(((got - ref).abs()[~z] / ref.abs()[~z]).max())


def fp32_bound_mask(Q, P):
    return 2.0 * (P + Q + 4) * U32


def fp32_bound_class(K1):
    return (K1 + 4) * U32


# ---- fixtures -------------------------------------------------------------------------------------------------------------------------
def _meta(z):
    return json.loads(bytes(z["meta"]).decode())


def unpack_bool(packed, shape):
    n = int(np.prod(shape))
    return torch.from_numpy(np.unpackbits(packed)[:n].astype(bool).reshape(shape))


class ShapeFixture:
    """inputs of one per-element case and, per (kind, masking) combination, the reference's fp32 results"""

    def __init__(self, s):
        self.shape = tuple(s)
        z = np.load(os.path.join(GOLDEN, shape_name(s) + ".npz"))
        self.meta = _meta(z)
        Q, M, K, T, H, W = s
        self.pred = torch.from_numpy(z["pred_masks"]).float()               # fp16 values
        self.logits = torch.from_numpy(z["pred_logits"]).float()
        self.labels = torch.from_numpy(z["labels"])
        self.targets = {"bool": unpack_bool(z["tgt_bool"], (M, T, H, W)), "float": torch.from_numpy(z["tgt_float"]).float()}
        self.ref_class_sim = torch.from_numpy(z["ref_class_sim"])
        self.combos = [tuple(c) for c in self.meta["combos"]]
        self.ref = {}
        for kind, mv in self.combos:
            k = f"{kind}_{mv}"
            self.ref[(kind, mv)] = {n: torch.from_numpy(z[f"{k}_{n}"]) for n in ("mask_sim", "cost", "rows", "cols", "dice", "cls", "cost64")}
        self._restated = {}

    def restated(self, kind, mv):
        """float64 restatement of one combination, computed once and shared"""
        if (kind, mv) not in self._restated:
            self._restated[(kind, mv)] = restate(self.pred, self.logits, self.targets[kind], self.labels, mv)
        return self._restated[(kind, mv)]

    def reference_error(self, kind, mv):
        """the reference's own fp32 error on this fixture: the largest relative error of its mask similarity, class similarity and cost"""
        ms, cs, C, _, _ = self.restated(kind, mv)
        r = self.ref[(kind, mv)]
        return max(rel_err(r["mask_sim"], ms), rel_err(self.ref_class_sim, cs), rel_err(r["cost"], C))


class E2EFixture:
    def __init__(self, name):
        z = np.load(os.path.join(GOLDEN, name + ".npz"))
        self.meta = m = _meta(z)
        T, H, W = m["T"], m["H"], m["W"]
        self.layers = [{"pred_masks": torch.from_numpy(z[f"pred_masks_{l}"]).float(), "pred_logits": torch.from_numpy(z[f"pred_logits_{l}"]).float()}
                       for l in range(m["L"])]
        self.targets = [{"labels": torch.from_numpy(z[f"labels_{b}"]), "masks": unpack_bool(z[f"tgt_{b}"], (mb, T, H, W))} for b, mb in enumerate(m["M"])]
        self.ref = [[{n: torch.from_numpy(z[f"{n}_{l}_{b}"]) for n in ("rows", "cols", "dice", "cls", "cost64")} for b in range(m["B"])]
                    for l in range(m["L"])]

    def outputs(self, device=None, dtype=None):
        """the dict the criterion hands the matcher: final prediction = the LAST layer, aux_outputs = the ones before it"""
        mv = lambda t: t if device is None else t.to(device)
        ls = [{"pred_masks": mv(o["pred_masks"]) if dtype is None else mv(o["pred_masks"]).to(dtype), "pred_logits": mv(o["pred_logits"])} for o in self.layers]
        return dict(ls[-1], aux_outputs=ls[:-1])

    def targets_on(self, device):
        return [{k: v.to(device) for k, v in t.items()} for t in self.targets]


_shape_cache = {}


def shape_fixture(s):
    s = tuple(s)
    if s not in _shape_cache:
        _shape_cache[s] = ShapeFixture(s)
    return _shape_cache[s]
