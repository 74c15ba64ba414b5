"""Tube-Link's point-sampled training loss on the device: `tube_link_losses` / `TubeLinkSetCriterion`.

Reference: MaXTron_Tube-Link/models/video/tube_link_vis/mask2former_video_cc_head.py:519-694 (`loss`, `loss_single`,
`_get_target_single`).  There, every (layer, video) pair samples all Q predictions and M targets at `num_points` random points, builds
the Q x M cost from three terms, copies it to the host for SciPy's assignment, and every layer then samples
`num_points * oversample_ratio` candidates per matched mask, keeps the most uncertain ones by top-k and evaluates three losses through
autograd.  Here the random coordinates are drawn up front in the reference's order (`draw_point_coords`), and one library call
computes the cost, the assignment, the selection and the losses of ALL layers; the backward is a second call.  What is kept in between
is O(L * G * num_points); the host is never synchronised.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence, Tuple

import torch
from torch import Tensor, nn
from torch.autograd.function import once_differentiable

from . import _lib
from ._autograd import cast, f32c, nbytes, place, require_gpu


def sample_counts(num_points: int, oversample_ratio: float, importance_sample_ratio: float) -> Tuple[int, int]:
    """(S, k): candidates per matched mask and how many of them are kept (mmdet/models/utils/point_sample.py:60, :74)."""
    if oversample_ratio < 1 or not 0 <= importance_sample_ratio <= 1:
        raise ValueError("need oversample_ratio >= 1 and 0 <= importance_sample_ratio <= 1")
    return int(num_points * oversample_ratio), int(importance_sample_ratio * num_points)


def draw_point_coords(L: int, m_per_video: Sequence[int], Q: int, num_points: int, oversample_ratio: float, importance_sample_ratio: float,
                      device, generator: Optional[torch.Generator] = None) -> Tuple[Tensor, Tensor, Tensor]:
    """The random coordinates of one `loss()` call, drawn with torch.rand in the reference's order and shapes: per layer (1, P, 2) per
    video (`_get_target_single`, also for a video without objects), then (G, S, 2) and, when P - k > 0, (G, P - k, 2)
    (`get_uncertain_point_coords_with_randomness`); a layer without a matched pair draws only the first.  G = sum_b min(Q, M_b).
    -> match_coords [L, B, P, 2], cand_coords [L, G, S, 2], rand_coords [L, G, P - k, 2]."""
    S, k = sample_counts(num_points, oversample_ratio, importance_sample_ratio)
    B, G, P = len(m_per_video), sum(min(Q, int(m)) for m in m_per_video), num_points
    match = torch.empty(L, B, P, 2, dtype=torch.float32, device=device)
    cand = torch.empty(L, G, S, 2, dtype=torch.float32, device=device)
    rand = torch.empty(L, G, P - k, 2, dtype=torch.float32, device=device)
    for l in range(L):
        for b in range(B):
            match[l, b] = torch.rand((1, P, 2), device=device, generator=generator)[0]
        if G > 0:
            cand[l] = torch.rand(G, S, 2, device=device, generator=generator)
            if P - k > 0:
                rand[l] = torch.rand(G, P - k, 2, device=device, generator=generator)
    return match, cand, rand


class _TubeLinkLoss(torch.autograd.Function):
    """(losses [L, 3], rows, cols[, cost, sel_idx]) of L layers' (cls_scores, mask_preds); targets, coordinates and the matched count are
    constants of the step."""

    @staticmethod
    def forward(ctx, cfg, tcat, lcat, cw, coords, ntm, debug, *preds):
        from .modules import _stream
        m, P, S, k, cost_w, loss_w, eps = cfg
        L = len(preds) // 2
        for t in preds:
            require_gpu(t)
        cls = [f32c(t) for t in preds[:L]]
        masks = [f32c(t) for t in preds[L:]]
        dev = masks[0].device
        B, T, Q, h, w = masks[0].shape
        K1 = cls[0].shape[-1]
        Hg, Wg = (int(tcat.shape[2]), int(tcat.shape[3])) if tcat is not None else (h, w)
        tdt = _lib.AXVS_F32 if (tcat is not None and tcat.dtype == torch.float32) else _lib.AXVS_U8
        c = _lib.AxvsTLLossCfg(L=L, B=B, Q=Q, K1=K1, T=T, h=h, w=w, Hg=Hg, Wg=Wg, num_points=P, num_cand=S, num_kept=k, target_dtype=tdt,
                               cost_cls=cost_w[0], cost_mask=cost_w[1], cost_dice=cost_w[2], loss_cls=loss_w[0], loss_mask=loss_w[1],
                               loss_dice=loss_w[2], dice_eps=eps)
        mv = (C.c_int * B)(*m)
        G, kmax = sum(min(Q, x) for x in m), min(Q, max(m))
        match, cand, rand = coords
        lib = _lib.lib()
        with torch.cuda.device(dev):
            losses = torch.empty(L, 3, dtype=torch.float32, device=dev)
            rows = torch.empty(L * B, kmax, dtype=torch.int64, device=dev)
            cols = torch.empty(L * B, kmax, dtype=torch.int64, device=dev)
            cost = torch.empty(L * B, Q, max(m), dtype=torch.float32, device=dev) if debug else None
            sel = torch.empty(L, G, k, dtype=torch.int32, device=dev) if debug else None
            saved, saved_ptr, scratch = place(dev, nbytes("axvs_tl_loss_saved_bytes", c, mv), nbytes("axvs_tl_loss_workspace_bytes", c, mv))
            ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()
            _lib.check(lib.axvs_tl_loss_fwd(c, _lib.ptrs(cls), _lib.ptrs(masks), ptr(tcat), ptr(lcat), mv, cw.data_ptr(), ptr(match), ptr(cand), ptr(rand),
                                            ntm.data_ptr(), losses.data_ptr(), ptr(rows), ptr(cols), ptr(cost), ptr(sel), saved_ptr,
                                            scratch.data_ptr(), scratch.numel(), _stream(dev)), "axvs_tl_loss_fwd")
        ctx.save_for_backward(saved, *cls, *masks)
        ctx.consts = (tcat, cw, ntm)            # constants of the step (no autograd history): kept alive for the backward
        ctx.cfg = (c, tuple(m), L)
        ctx.in_dtypes = [t.dtype for t in preds]
        ctx.in_shapes = [tuple(t.shape) for t in preds]
        extra = (rows, cols) + ((cost, sel) if debug else ())
        ctx.mark_non_differentiable(*extra)
        return (losses,) + extra

    @staticmethod
    @once_differentiable
    def backward(ctx, d_losses, *_):
        from .modules import _stream
        saved, *ts = ctx.saved_tensors
        c, m, L = ctx.cfg
        tcat, cw, ntm = ctx.consts
        cls, masks = ts[:L], ts[L:]
        dev = saved.device
        g = f32c(d_losses)
        with torch.cuda.device(dev):
            need = ctx.needs_input_grad[7:]
            dc = [torch.empty_like(x) if need[i] else None for i, x in enumerate(cls)]
            dm = [torch.empty_like(x) if need[L + i] else None for i, x in enumerate(masks)]
            _lib.check(_lib.lib().axvs_tl_loss_bwd(c, g.data_ptr(), _lib.ptrs(cls), _lib.ptrs(masks), None if tcat is None else tcat.data_ptr(),
                                                   (C.c_int * len(m))(*m), cw.data_ptr(), ntm.data_ptr(), saved.data_ptr(), _lib.ptrs(dc), _lib.ptrs(dm),
                                                   _stream(dev)), "axvs_tl_loss_bwd")
        grads = [None if d is None else d.reshape(s) for d, s in zip(dc + dm, ctx.in_shapes)]
        return (None,) * 7 + tuple(cast(grads, ctx.in_dtypes))


def _layers(x, what: str) -> List[Tensor]:
    ts = list(x.unbind(0)) if isinstance(x, Tensor) else list(x)
    if not ts:
        raise ValueError(f"{what}: no decoder layer")
    for t in ts:
        if t.dtype != torch.float32:
            raise NotImplementedError(f"axial_vs_amd: {what} must be fp32 (got {t.dtype}): the reference's @force_fp32 makes them so, and "
                                      "16-bit mask inputs are not built")
        if not t.is_cuda:
            raise RuntimeError(f"axial_vs_amd: {what} must be GPU tensors (got {t.device}); there is no CPU fallback")
        if t.shape != ts[0].shape:
            raise RuntimeError(f"{what}: every layer must have the same shape")
    return ts


def tube_link_losses(all_cls_scores, all_mask_preds, gt_labels_list: Sequence[Tensor], gt_masks_list: Sequence[Tensor], *, num_classes: int,
                     class_weight, num_points: int = 12544, oversample_ratio: float = 3.0, importance_sample_ratio: float = 0.75,
                     cost_weights=(2., 5., 5.), loss_weights=(2., 5., 5.), dice_eps: float = 1.0, point_coords=None,
                     generator: Optional[torch.Generator] = None, reduce_mean=None, return_assignment: bool = False):
    """`Mask2FormerVideoCCHeadTube.loss` on the device -> mmdet's dict of 0-dim fp32 tensors: loss_cls / loss_mask / loss_dice of the LAST
    layer, d{i}.loss_* of layer i before it (mask2former_video_cc_head.py:583-596), differentiable with respect to every layer's
    cls_scores [B, Q, K + 1] and mask_preds [B, T, Q, h, w] (fp32, on the GPU; a tensor with a leading layer axis or a sequence).

    gt_labels_list / gt_masks_list: per video int64 [M_b] and bool / uint8 / fp32 [M_b, T, Hg, Wg] on the GPU (any resolution: the
    coordinates are normalised).  class_weight: K + 1 weights.  cost_weights / loss_weights: (class, mask, dice).  point_coords: the
    result of `draw_point_coords` (drawn here from `generator` otherwise).  reduce_mean: applied to the device scalar of the matched
    count before it is clamped to 1 (the reference's `reduce_mean`).  Q <= 512, M_b <= 512, num_points <= 16384,
    int(num_points * oversample_ratio) <= 65536, T * h <= 8192.  A label outside 0 .. K-1 is clamped (the reference raises).
    Among candidates of equal |logit| the lower index is kept, where the reference's topk leaves the order open.

    return_assignment: -> (dict, info) with info = {"rows", "cols": int64 [L * B, min(Q, max M_b)] as SciPy returns them (-1 pads),
    "cost": fp32 [L * B, Q, max M_b], "selected": int32 [L, G, k] kept candidates in increasing order, "point_coords"}."""
    cls, masks = _layers(all_cls_scores, "all_cls_scores"), _layers(all_mask_preds, "all_mask_preds")
    L = len(cls)
    if len(masks) != L or masks[0].dim() != 5 or cls[0].dim() != 3:
        raise RuntimeError("need L layers of cls_scores [B, Q, K + 1] and mask_preds [B, T, Q, h, w]")
    B, T, Q, h, w = masks[0].shape
    K1 = cls[0].shape[-1]
    if K1 != num_classes + 1 or cls[0].shape[:2] != (B, Q):
        raise RuntimeError(f"cls_scores {tuple(cls[0].shape)} does not fit mask_preds {tuple(masks[0].shape)} and num_classes = {num_classes}")
    if len(gt_labels_list) != B or len(gt_masks_list) != B:
        raise RuntimeError(f"{len(gt_labels_list)} label and {len(gt_masks_list)} mask entries for a batch of {B}")
    dev = masks[0].device
    S, k = sample_counts(num_points, oversample_ratio, importance_sample_ratio)
    m = [int(t.shape[0]) for t in gt_labels_list]
    with torch.cuda.device(dev), torch.no_grad():
        tcat = lcat = None
        if max(m) > 0:
            gm = [t for t in gt_masks_list if t.shape[0] > 0]
            for t, n in zip(gt_masks_list, m):
                if t.shape[0] != n or not t.is_cuda or (n > 0 and (t.dim() != 4 or t.shape[1] != T or t.shape[2:] != gm[0].shape[2:])):
                    raise RuntimeError("gt_masks_list: per video a GPU tensor [M_b, T, Hg, Wg] with M_b = len(gt_labels)")
            tcat = torch.cat(gm, 0)
            if tcat.dtype == torch.bool:
                tcat = tcat.view(torch.uint8)
            elif tcat.dtype not in (torch.uint8, torch.float32):
                raise NotImplementedError(f"axial_vs_amd: ground-truth masks must be bool, uint8 or fp32 (got {tcat.dtype})")
            tcat = tcat.contiguous()
            lcat = torch.cat([t.to(device=dev, dtype=torch.int64) for t in gt_labels_list if t.shape[0] > 0]).contiguous()
        cw = torch.as_tensor(class_weight, dtype=torch.float32).to(dev).contiguous()
        if cw.numel() != K1:
            raise RuntimeError(f"class_weight has {cw.numel()} entries for K + 1 = {K1} classes")
        if point_coords is None:
            point_coords = draw_point_coords(L, m, Q, num_points, oversample_ratio, importance_sample_ratio, dev, generator)
        G = sum(min(Q, x) for x in m)
        coords = tuple(f32c(t) for t in point_coords)
        if tuple(coords[0].shape) != (L, B, num_points, 2) or tuple(coords[1].shape) != (L, G, S, 2) or tuple(coords[2].shape) != (L, G, num_points - k, 2):
            raise RuntimeError("point_coords: need match [L, B, P, 2], cand [L, G, S, 2] and rand [L, G, P - k, 2] (draw_point_coords)")
        ntm = torch.full((1,), float(G), dtype=torch.float32, device=dev)
        if reduce_mean is not None:
            ntm = reduce_mean(ntm)
        ntm = ntm.clamp(min=1.0).float().contiguous()
    cfg = (m, int(num_points), S, k, tuple(float(x) for x in cost_weights), tuple(float(x) for x in loss_weights), float(dice_eps))
    with torch.cuda.device(dev), torch.autocast(device_type="cuda", enabled=False):
        out = _TubeLinkLoss.apply(cfg, tcat, lcat, cw, coords, ntm, bool(return_assignment), *cls, *masks)
    flat = out[0].reshape(-1)
    losses: Dict[str, Tensor] = {}
    for j, name in enumerate(("loss_cls", "loss_mask", "loss_dice")):
        losses[name] = flat[3 * (L - 1) + j]
    for i in range(L - 1):
        for j, name in enumerate(("loss_cls", "loss_mask", "loss_dice")):
            losses[f"d{i}.{name}"] = flat[3 * i + j]
    if not return_assignment:
        return losses
    return losses, {"rows": out[1], "cols": out[2], "cost": out[3], "selected": out[4], "point_coords": coords}


def _cfg_get(cfg, key, default=None):
    return default if cfg is None else (cfg.get(key, default) if hasattr(cfg, "get") else getattr(cfg, key, default))


def _expect(cfg, what: str, **want):
    for key, v in want.items():
        got = _cfg_get(cfg, key, v)
        if got != v:
            raise NotImplementedError(f"axial_vs_amd: {what} with {key} = {got!r} is not built: the device loss computes {key} = {v!r}")


class TubeLinkSetCriterion(nn.Module):
    """The loss of `Mask2FormerVideoCCHeadTube` built from the head's own config values; `loss(all_cls_scores, all_mask_preds,
    gt_labels_list, gt_masks_list, img_metas=None)` is a drop-in for the head's method and returns the same dict.

    loss_cls / loss_mask / loss_dice / train_cfg are the head's config dicts (models/video/tube_link_vis/mask2former_video_cc_head.py:
    304-409; configs/video/_base_/models/mask2former_tube_r50.py).  Only what the shipped configs use is built -- softmax
    CrossEntropyLoss with class_weight, sigmoid CrossEntropyLoss, the naive activated DiceLoss, MaskHungarianAssigner with
    ClassificationCost + CrossEntropyLossCost + DiceCost(pred_act, naive), MaskPseudoSampler, point_loss=True -- and anything else
    raises NotImplementedError at construction instead of falling back to torch.  `reduce_mean`: the function applied to the matched
    count (mmdet.core.reduce_mean in a distributed run; None on one process)."""

    def __init__(self, num_classes: int, loss_cls=None, loss_mask=None, loss_dice=None, train_cfg=None, point_loss: bool = True, reduce_mean=None):
        super().__init__()
        if not point_loss:
            raise NotImplementedError("axial_vs_amd: point_loss=False (dense nearest-neighbour targets) is not built: the device loss samples points")
        _expect(loss_cls, "loss_cls", type="CrossEntropyLoss", use_sigmoid=False, reduction="mean")
        _expect(loss_mask, "loss_mask", type="CrossEntropyLoss", use_sigmoid=True, reduction="mean")
        _expect(loss_dice, "loss_dice", type="DiceLoss", use_sigmoid=True, activate=True, reduction="mean", naive_dice=True)
        asg = _cfg_get(train_cfg, "assigner")
        _expect(asg, "train_cfg.assigner", type="MaskHungarianAssigner")
        _expect(_cfg_get(asg, "cls_cost"), "cls_cost", type="ClassificationCost")
        _expect(_cfg_get(asg, "mask_cost"), "mask_cost", type="CrossEntropyLossCost", use_sigmoid=True)
        _expect(_cfg_get(asg, "dice_cost"), "dice_cost", type="DiceCost", pred_act=True, naive_dice=True)
        _expect(_cfg_get(train_cfg, "sampler"), "train_cfg.sampler", type="MaskPseudoSampler")
        self.num_classes = int(num_classes)
        cw = _cfg_get(loss_cls, "class_weight")
        self.class_weight = [1.0] * (self.num_classes + 1) if cw is None else [float(x) for x in cw]
        if len(self.class_weight) != self.num_classes + 1:
            raise ValueError(f"loss_cls.class_weight has {len(self.class_weight)} entries for num_classes + 1 = {self.num_classes + 1}")
        self.loss_weights = (float(_cfg_get(loss_cls, "loss_weight", 2.0)), float(_cfg_get(loss_mask, "loss_weight", 5.0)),
                             float(_cfg_get(loss_dice, "loss_weight", 5.0)))
        self.cost_weights = (float(_cfg_get(_cfg_get(asg, "cls_cost"), "weight", 2.0)), float(_cfg_get(_cfg_get(asg, "mask_cost"), "weight", 5.0)),
                             float(_cfg_get(_cfg_get(asg, "dice_cost"), "weight", 5.0)))
        self.dice_eps = float(_cfg_get(loss_dice, "eps", 1.0))
        cost_eps = float(_cfg_get(_cfg_get(asg, "dice_cost"), "eps", 1.0))
        if cost_eps != self.dice_eps:
            raise NotImplementedError(f"axial_vs_amd: DiceCost eps = {cost_eps} and DiceLoss eps = {self.dice_eps} differ: the device loss takes one eps")
        self.num_points = int(_cfg_get(train_cfg, "num_points", 12544))
        self.oversample_ratio = float(_cfg_get(train_cfg, "oversample_ratio", 3.0))
        self.importance_sample_ratio = float(_cfg_get(train_cfg, "importance_sample_ratio", 0.75))
        self.point_loss = True
        self.reduce_mean = reduce_mean
        self._cw_on = {}                 # device -> class_weight there (copied once: a host-to-device copy per step would wait for the stream)
        sample_counts(self.num_points, self.oversample_ratio, self.importance_sample_ratio)

    def loss(self, all_cls_scores, all_mask_preds, gt_labels_list, gt_masks_list, img_metas=None, generator=None):
        dev = all_mask_preds[0].device
        if dev not in self._cw_on:
            self._cw_on[dev] = torch.tensor(self.class_weight, dtype=torch.float32, device=dev)
        return tube_link_losses(all_cls_scores, all_mask_preds, gt_labels_list, gt_masks_list, num_classes=self.num_classes,
                                class_weight=self._cw_on[dev], num_points=self.num_points, oversample_ratio=self.oversample_ratio,
                                importance_sample_ratio=self.importance_sample_ratio, cost_weights=self.cost_weights,
                                loss_weights=self.loss_weights, dice_eps=self.dice_eps, generator=generator, reduce_mean=self.reduce_mean)

    forward = loss

    def extra_repr(self) -> str:
        return (f"num_classes={self.num_classes}, num_points={self.num_points}, oversample_ratio={self.oversample_ratio}, "
                f"importance_sample_ratio={self.importance_sample_ratio}, cost_weights={self.cost_weights}, loss_weights={self.loss_weights}")
