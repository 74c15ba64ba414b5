"""The sampled pixel losses of the within-clip criterion (axial_vs_amd.sampled_pixel_losses / MaXTronWCSetCriterion): a float64
restatement of the reference's `pixels` and `aux_semantic` losses (MaXTron_Video-kMaX/maxtron_deeplab/modeling/wc_criterion.py:62-142,
:271-305, :341-415) in plain torch, the case tables, the screen, the fixture reader and the error measures shared by
tests/test_pixel_losses_cpu.py, tests/test_hip_pixel_losses.py and tools/gen_golden_pixel_losses.py.

RESTATEMENT (all float64, on the fixture's stored inputs and its stored uniform noise u).  Per matching j (one when the final matching
is shared, else one per layer) and video b, with (rows, cols) the matched pairs and P = T*H*W:
    t[rows] = masks[cols], 0 elsewhere;  area[n] = sum_p t[n,p];  pix_area[p] = sum_n t[n,p] area[n];  void[p] = sum_n t[n,p] < 1
    key[p]  = log(P / max(pix_area[p], 1)) * temperature + void[p] * (-99999) + (-log(-log u[p]))
    samples = the k largest keys of the row (a set: both losses are sums over it)
    loss_pixel_insdis (layer l):  F = pixel_feature[l][b][:, samples], G = t[:, samples], S = F^T F / 0.3, g = G^T G,
        c_j = sum_k g[k,j], q = g / max(c_j, 1), loss_j = -sum_k q[k,j] log_softmax_k(S[k,j]);  mean_b sum_j loss_j / max(#{loss_j != 0}, 1)
    loss_aux_semantic (final prediction, its own noise / temperature / k):  cross-entropy of aux_semantic_pred[b][:, p] against
        semantic_masks[b][p] at the samples, -1 -> num_classes = ignored, the same nonzero-count mean
Noise rows: u_pixels[l] for layer l (layer 0 = the final prediction, 1 + i = aux_outputs[i]) and u_semantic, drawn by torch.rand in
the order final `pixels`, final `aux_semantic`, aux `pixels` 0, 1, ...  Gradients come from autograd on this.

ERROR MEASURES.  A loss scalar: |got - ref| / |ref|.  A gradient tensor: max|got - ref| / max|ref|.

THE YARDSTICK of the GPU test is the reference's own fp32 CPU result against this restatement, per fixture, taken separately over the
loss scalars and over the gradient tensors, floored at 2^-24: the device may be 8 times as far from float64 (the project's margin).

THE BOUND of the CPU test on the reference's fp32 values comes from the number format (u = 2^-24): an element of S is a sum of C
products scaled by 1 / 0.3 ((C + 2) u), a log-softmax over k values carries (k + 4) u more, loss_j is a sum of at most k such terms
weighted by q (k u), the sum over j and the division by the count add (k + 1) u; the semantic loss is the same with Cs for C and no
inner sum: fp32_bound = 4 (C + 3 k + 8) u, relative to the value for a scalar and to the largest entry for a gradient.

THE SCREEN.  A noise seed is kept only if, in float64, the k-th and the (k + 1)-th largest key of EVERY row are further apart than 8
times the largest |fp32 key - float64 key| of the reference on that row (measured by the generator on the keys the reference hands
`torch.topk`), so no fp32 evaluation of the keys can select another set.  A row with k = P has no (k + 1)-th key and passes.  The
matcher's pairs are screened as in criterion_cases (equal to the float64 optimum and stable).  Void pixels carry keys near -99999,
where fp32 resolves 0.0078: a screened row never reaches them.  UNSCREENED_CASES has fewer non-void pixels than k, so void pixels
must be taken and the fp32 keys tie: the tests assert the selection rule (every non-void pixel, then void ones, equal keys to the
lower index) and compare the losses with the restatement on the device's own sample set.

CASES sit at the edges of the kernels' guard code.  A workgroup of the streamed kernels owns 16 columns and its 4 waves walk the
16-row tiles of k in turn (a round of 64 rows), the contraction runs in steps of 16 channels / matched pairs (zero padded), the
backward keeps its gradient tile in registers sized for C <= 128 or for C <= 256, a wave of the select owns a contiguous range of
64-pixel chunks:
    k1            k = 1: one valid row, three row groups of wave 0 and the other three waves empty; C = 4 (padded to 16)
    k63 / k64 / k65   one below, at and one above a round of the four waves (the last column tile partial, full, a fifth tile of one
                  column; wave 0 alone has a second row tile at 65); C = 20 (16 + 4: a padded second step); L = 2, shared matching
    own           own matching per layer, B = 2 with M = (4, 2); k = 65.  Six (row, video) pairs have to pass the screen at once, and a
                  void pixel's fp32 key is 0.004 to 0.008 off, which asks for a gap of 0.06 where the mean gap is 0.02: this case and
                  P1100 use targets without void pixels (kind "boolfull": the first object also owns what no object owns)
    k145_C128     two rounds and a remainder of 17 rows (ten column tiles, the last with one column); C = 128: the smaller backward's top
    C132          C = 132: the first C of the larger backward (nine channel blocks, the last with four channels)
    kP            k = P: every pixel
    M0            a video without objects (all void: insdis exactly 0 there, semantic loss not), k = P so that its void keys are all taken
    MgtN          M = 7 > N = 4: only four targets are matched
    float         overlapping float targets (g through the fp32 contraction)
    semignore     a semantic map that is entirely -1: loss_aux_semantic exactly 0
    P1100         P = 1100: 17 chunks and 12 pixels over the select's waves, more than one 1024-pixel stride; L = 3, k = 300 / 257
"""
import json
import os

import numpy as np
import torch

import criterion_cases as cc
import matcher_cases as mc

GOLDEN = mc.GOLDEN
U32 = mc.U32
FLOOR = 2.0 ** -24
MARGIN = 8.0
VOID_LOGIT = -99999.0
TAU = 0.3
SEEDS = os.path.join(GOLDEN, "g25_pixel_losses_seeds.json")

# name: (N, objects per video, K, T, H, W, layers, share_final_matching, target kind, C, k_pixels, k_semantic, semantic kind)
CASES = {
    "g25_pixel_losses_k1": (8, (3,), 5, 1, 9, 13, 1, 1, "bool", 4, 1, 1, "rand"),
    "g25_pixel_losses_k63": (8, (3,), 5, 2, 9, 13, 2, 1, "bool", 20, 63, 64, "rand"),
    "g25_pixel_losses_k64": (8, (3,), 5, 2, 9, 13, 1, 1, "bool", 20, 64, 65, "rand"),
    "g25_pixel_losses_k65_own": (8, (4, 2), 5, 2, 9, 13, 2, 0, "boolfull", 8, 65, 63, "rand"),
    "g25_pixel_losses_k145_C128": (16, (5,), 7, 2, 12, 17, 1, 1, "bool", 128, 145, 145, "rand"),
    "g25_pixel_losses_C132": (8, (3,), 5, 1, 9, 13, 1, 1, "bool", 132, 20, 20, "rand"),
    "g25_pixel_losses_kP": (8, (3,), 5, 1, 9, 13, 1, 1, "bool", 8, 117, 117, "rand"),
    "g25_pixel_losses_M0": (8, (3, 0), 5, 1, 9, 13, 2, 1, "bool", 8, 117, 117, "rand"),
    "g25_pixel_losses_MgtN": (4, (7,), 5, 2, 9, 13, 1, 1, "bool", 8, 40, 40, "rand"),
    "g25_pixel_losses_float": (8, (4,), 5, 2, 9, 13, 2, 1, "float", 12, 24, 24, "rand"),
    "g25_pixel_losses_semignore": (8, (3,), 5, 1, 9, 13, 1, 1, "bool", 4, 20, 20, "ignore"),
    "g25_pixel_losses_P1100": (8, (6,), 9, 2, 22, 25, 3, 1, "boolfull", 16, 300, 257, "rand"),
}
# fewer non-void pixels than k: no screened fixture exists (see THE SCREEN)
UNSCREENED_CASES = {
    "sparse_k40": (8, (2,), 5, 2, 9, 13, 2, 1, "sparse", 8, 40, 40, "rand"),
}
TEMPERATURES = (1.8, 2.4)          # pixel_insdis_temperature, aux_semantic_temperature of the within-clip configs


def loss_keys(L, pixels=True, semantic=True):
    """the reference's result keys for losses = ["pixels", "aux_semantic"], in its order"""
    keys = []
    for l in range(L):
        if pixels:
            keys.append("loss_pixel_insdis" if l == 0 else f"loss_pixel_insdis_{l - 1}")
        if semantic and l == 0:
            keys.append("loss_aux_semantic")
    return keys


def make_case(case, seed):
    """inputs of a case (fp16-representable fp32): layers [{pred_masks, pred_logits, pixel_feature [B, C, T, H, W]}], layer 0 also
    aux_semantic_pred [B, K, T, H, W]; targets [{labels, masks, semantic_masks int64 [T, H, W]}]"""
    N, Ms, K, T, H, W, L, share, kind, C, kp, ks, semkind = case
    base_kind = {"sparse": "bool", "boolfull": "bool"}.get(kind, kind)
    layers, targets = cc.make_case((N, Ms, K, T, H, W, L, share, 1, base_kind), seed)
    g = torch.Generator().manual_seed(25000 + seed)
    B = len(Ms)
    for b, t in enumerate(targets):
        if kind == "sparse":        # objects of five pixels each: far fewer non-void pixels than k
            m = torch.zeros_like(t["masks"]).flatten(1)
            perm = torch.randperm(m.shape[1], generator=g)
            for i in range(m.shape[0]):
                m[i, perm[5 * i:5 * i + 5]] = True
            t["masks"] = m.reshape(t["masks"].shape)
        if kind == "boolfull" and t["masks"].shape[0]:        # no void pixel: the first object takes what no object owns
            t["masks"] = t["masks"].clone()
            t["masks"][0] |= ~t["masks"].any(0)
        sem = torch.randint(-1, K, (T, H, W), generator=g)
        t["semantic_masks"] = torch.full_like(sem, -1) if semkind == "ignore" else sem
    for l, o in enumerate(layers):
        o["pixel_feature"] = (torch.randn(B, C, T, H, W, generator=g) * 0.5).half().float()
    layers[0]["aux_semantic_pred"] = (torch.randn(B, K, T, H, W, generator=g) * 2.0).half().float()
    return layers, targets


# ---- float64 restatement ------------------------------------------------------------------------------------------------------------
def padded_targets64(N, P, tgt, rows, cols):
    t = torch.zeros(N, P, dtype=torch.float64)
    if rows.numel():
        t[rows] = tgt["masks"].double().flatten(1)[cols]
    return t


def keys64(t, u, temperature):
    """-> key float64 [P], void bool [P]"""
    P = t.shape[1]
    area = t.sum(1)
    pix = (t * area[:, None]).sum(0)
    void = t.sum(0) < 1
    inv = P / pix.clamp(min=1.0)
    return torch.log(inv) * temperature + void.double() * VOID_LOGIT + (-torch.log(-torch.log(u.double()))), void


def topk_set(key, k):
    """the k largest keys as an increasing index vector (int64)"""
    return torch.topk(key, k).indices.sort().values if k > 0 else torch.zeros(0, dtype=torch.int64)


def gap_at(key, k):
    """distance between the k-th and the (k + 1)-th largest key (inf when there is none)"""
    if k <= 0 or k >= key.numel():
        return float("inf")
    v = torch.topk(key, k + 1).values
    return float(v[k - 1] - v[k])


def insdis64(F, t, idx):
    """F float64 [C, P], t [N, P], idx int64 [k] -> the video's sum_j loss_j / max(#nonzero, 1)"""
    if idx.numel() == 0:
        return F.sum() * 0.0
    f, G = F[:, idx], t[:, idx]
    S = f.T @ f / TAU
    g = G.T @ G
    q = g / g.sum(0, keepdim=True).clamp(min=1.0)
    loss = -(q * torch.log_softmax(S, 0)).sum(0)
    return loss.sum() / max(int((loss != 0).sum()), 1)


def semantic64(x, sem, idx, num_classes):
    """x float64 [Cs, P], sem int64 [P] -> the video's sum / max(#nonzero, 1)"""
    if idx.numel() == 0:
        return x.sum() * 0.0
    tg = sem[idx].clone()
    tg[tg == -1] = num_classes
    keep = tg != num_classes
    xs = x[:, idx]
    lse = torch.logsumexp(xs, 0)
    picked = xs[tg.clamp(max=xs.shape[0] - 1), torch.arange(idx.numel())]
    loss = (lse - picked) * keep.double()
    return loss.sum() / max(int((loss != 0).sum()), 1)


def row_plan(L, share, kp, ks, pixels=True, semantic=True):
    """[(kind, layer, matching, temperature index, k)] of the noise rows: the L `pixels` rows, then the `aux_semantic` row"""
    rows = [("pixels", l, 0 if share else l, 0, kp) for l in range(L)] if pixels else []
    return rows + ([("aux_semantic", 0, 0, 1, ks)] if semantic else [])


def sample_sets64(N, P, targets, pairs, share, L, kp, ks, u_pix, u_sem, temperatures=TEMPERATURES):
    """-> per noise row and video: (idx int64 increasing, key float64 [P], void [P], gap)"""
    out = []
    for kind, l, j, ti, k in row_plan(L, share, kp, ks):
        per = []
        for b, tgt in enumerate(targets):
            t = padded_targets64(N, P, tgt, *pairs[j][b])
            u = u_pix[l, b] if kind == "pixels" else u_sem[b]
            key, void = keys64(t, u, temperatures[ti])
            per.append((topk_set(key, k), key, void, gap_at(key, k)))
        out.append(per)
    return out


def losses64(layers, targets, pairs, N, K, share, samples):
    """-> {key: float64 scalar} in the reference's order.  layers: float64 leaves; samples[r][b] = index vector (the rows of row_plan)"""
    L, B = len(layers), len(targets)
    P = layers[0]["pixel_feature"][0, 0].numel()
    out = {}
    for l in range(L):
        j = 0 if share else l
        tot = 0.0
        for b in range(B):
            t = padded_targets64(N, P, targets[b], *pairs[j][b])
            tot = tot + insdis64(layers[l]["pixel_feature"][b].flatten(1), t, samples[l][b])
        out["loss_pixel_insdis" if l == 0 else f"loss_pixel_insdis_{l - 1}"] = tot / B
        if l == 0:
            tot = 0.0
            for b in range(B):
                tot = tot + semantic64(layers[0]["aux_semantic_pred"][b].flatten(1), targets[b]["semantic_masks"].reshape(-1), samples[L][b], K)
            out["loss_aux_semantic"] = tot / B
    return out


def upstream_weights(n):
    return [1.0 + 0.1 * i for i in range(n)]


scalar_err, grad_err = cc.scalar_err, cc.grad_err


def fp32_bound(C, k):
    return 4.0 * (C + 3 * k + 8) * U32


# ---- fixtures -------------------------------------------------------------------------------------------------------------------------
class PixelLossFixture:
    """inputs of one case, the stored noise, the reference's fp32 losses / gradients / sample sets, and the float64 restatement"""

    def __init__(self, name):
        self.name = name
        z = np.load(os.path.join(GOLDEN, name + ".npz"))
        self.meta = m = json.loads(bytes(z["meta"]).decode())
        self.N, self.K, self.L, self.B, self.C = m["N"], m["K"], m["L"], len(m["M"]), m["C"]
        self.kp, self.ks, self.share, self.kind = m["kp"], m["ks"], bool(m["share"]), m["kind"]
        shp = (m["T"], m["H"], m["W"])
        self.P = shp[0] * shp[1] * shp[2]
        self.layers = []
        for l in range(self.L):
            o = {k: torch.from_numpy(z[f"{k}_{l}"]).float() for k in ("pred_masks", "pred_logits", "pixel_feature")}
            if l == 0:
                o["aux_semantic_pred"] = torch.from_numpy(z["aux_semantic_pred"]).float()
            self.layers.append(o)
        self.targets = []
        for b, mb in enumerate(m["M"]):
            masks = mc.unpack_bool(z[f"tgt_{b}"], (mb,) + shp) if self.kind in ("bool", "boolfull") else torch.from_numpy(z[f"tgt_{b}"]).float()
            self.targets.append({"labels": torch.from_numpy(z[f"labels_{b}"]), "masks": masks,
                                 "semantic_masks": torch.from_numpy(z[f"sem_{b}"]).to(torch.int64)})
        nm = 1 if self.share else self.L
        self.pairs = [[(torch.from_numpy(z[f"rows_{j}_{b}"]), torch.from_numpy(z[f"cols_{j}_{b}"])) for b in range(self.B)] for j in range(nm)]
        self.u_pix, self.u_sem = torch.from_numpy(z["u_pix"]), torch.from_numpy(z["u_sem"])
        self.keys = loss_keys(self.L)
        self.ref_losses = {k: float(v) for k, v in zip(self.keys, z["ref_losses"])}
        self.ref_dfeat = [torch.from_numpy(z[f"ref_dfeat_{l}"]) for l in range(self.L)]
        self.ref_dsem = torch.from_numpy(z["ref_dsem"])
        # the reference's sample sets, increasing: rows of row_plan
        self.ref_samples = [[torch.from_numpy(z[f"ref_idx_{r}_{b}"]).to(torch.int64) for b in range(self.B)] for r in range(self.L + 1)]
        self._sets = None
        self._restated = {}

    def outputs(self, device=None, requires_grad=False):
        ls = []
        for o in self.layers:
            d = {}
            for k, v in o.items():
                v = (v if device is None else v.to(device)).clone()
                d[k] = v.requires_grad_(requires_grad and k in ("pixel_feature", "aux_semantic_pred"))
            ls.append(d)
        return dict(ls[0], aux_outputs=ls[1:]) if self.L > 1 else dict(ls[0])

    def targets_on(self, device):
        return [{k: v.to(device) for k, v in t.items()} for t in self.targets]

    def noise_on(self, device):
        return self.u_pix.to(device), self.u_sem.to(device)

    def sets64(self):
        if self._sets is None:
            self._sets = sample_sets64(self.N, self.P, self.targets, self.pairs, self.share, self.L, self.kp, self.ks, self.u_pix, self.u_sem)
        return self._sets

    def restated(self, weights=None, samples=None):
        """({key: float64 loss}, d pixel_feature per layer, d aux_semantic_pred) of sum_i w_i loss_i on the float64 sample sets (or `samples`)"""
        key = (None if weights is None else tuple(weights), None if samples is None else id(samples))
        if key not in self._restated:
            ls = [{k: v.double().requires_grad_(k in ("pixel_feature", "aux_semantic_pred")) for k, v in o.items()} for o in self.layers]
            sm = samples if samples is not None else [[s[0] for s in per] for per in self.sets64()]
            losses = losses64(ls, self.targets, self.pairs, self.N, self.K, self.share, sm)
            w = [1.0] * len(losses) if weights is None else list(weights)
            total = sum(wi * v for wi, v in zip(w, losses.values()))
            if total.requires_grad:
                total.backward()
            zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
            self._restated[key] = ({k: v.detach() for k, v in losses.items()}, [zero(o["pixel_feature"]) for o in ls], zero(ls[0]["aux_semantic_pred"]))
        return self._restated[key]

    def reference_errors(self):
        """the reference's own fp32 errors against the restatement: (largest over the loss scalars, largest over the gradient tensors)"""
        losses, df, ds = self.restated()
        el = max(scalar_err(self.ref_losses[k], losses[k]) for k in self.keys)
        eg = max([grad_err(self.ref_dfeat[l], df[l]) for l in range(self.L)] + [grad_err(self.ref_dsem, ds)])
        return el, eg

    def yard(self):
        el, eg = self.reference_errors()
        return max(el, FLOOR), max(eg, FLOOR)


_cache = {}


def fixture(name):
    if name not in _cache:
        _cache[name] = PixelLossFixture(name)
    return _cache[name]
