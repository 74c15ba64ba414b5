"""The set criterion of the Video-kMaX models on the device: `MaXTronCCSetCriterion` / `MaXTronWCSetCriterion`.

Reference: MaXTron_Video-kMaX/maxtron_deeplab/modeling/cc_criterion.py:203-453 (wc_criterion.py is the same class without
`clip_outputs`).  There, every layer scatters the ground truth into a zero tensor shaped like pred_masks, takes a softmax over the
queries for the void IoU, again for the dice term, a log-softmax for the mask cross-entropy, and autograd keeps those maps.  Here the
matcher's indices stay on the GPU (matching.py), the `labels` and `masks` losses of ALL layers come out of one library call that reads
pred_masks once, the backward reads it once more and writes the gradient once, and what is kept in between is O(L * B * N).  No
[B, N, P] temporary exists besides the gradient, and the host is never synchronised.

The `'pixels'` and `'aux_semantic'` losses draw Gumbel noise and are requested by no shipped model (maxtron_cc_model.py:147,
maxtron_wc_model.py:130 hard-code ["labels", "masks"]): they are refused at construction.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional

import torch
from torch import Tensor, nn
from torch.autograd.function import once_differentiable

from . import _lib
from ._autograd import cast, f32c, nbytes, place, require_gpu
from .matching import _cat_targets, _device_of, _final_layer, _run_matcher

LOSS_KEYS = {"labels": ("loss_ce",), "masks": ("loss_mask", "loss_dice")}
_SLOT = {"loss_ce": 0, "loss_mask": 1, "loss_dice": 2}


def _ptrs(ts) -> C.Array:
    return (C.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


class _SetCriterion(torch.autograd.Function):
    """losses [L, 3] (loss_ce, loss_mask, loss_dice per layer) of L layers' (pred_masks, pred_logits); the matcher's results and the
    ground truth are constants (process_gt runs under no_grad on detached masks)."""

    @staticmethod
    def forward(ctx, cfg, tcat, lcat, rows, cols, dice, cls, *preds):
        from .modules import _stream
        m, kmax, K1, masking, share = cfg
        L = len(preds) // 2
        for t in preds:
            require_gpu(t)
        masks = [f32c(t).flatten(2) for t in preds[:L]]
        logits = [f32c(t) for t in preds[L:]]
        dev = masks[0].device
        B, N, P = masks[0].shape
        lib = _lib.lib()
        tdt = _lib.AXVS_F32 if (tcat is not None and tcat.dtype == torch.float32) else _lib.AXVS_U8
        with torch.cuda.device(dev):
            losses = torch.empty(L, 3, dtype=torch.float32, device=dev)
            saved, saved_ptr, scratch = place(dev, nbytes("axvs_set_criterion_saved_bytes", L, B, N),
                                              nbytes("axvs_set_criterion_workspace_bytes", L, B, N, K1, P))
            mv = (C.c_int * B)(*m)
            _lib.check(lib.axvs_set_criterion_fwd(_ptrs(masks), _ptrs(logits), None if tcat is None else tcat.data_ptr(), tdt,
                                                  None if lcat is None else lcat.data_ptr(), mv, rows.data_ptr(), cols.data_ptr(), dice.data_ptr(),
                                                  cls.data_ptr(), kmax, L, B, N, K1, P, int(masking), int(share), losses.data_ptr(), saved_ptr,
                                                  scratch.data_ptr(), scratch.numel(), _stream(dev)), "axvs_set_criterion_fwd")
        ctx.save_for_backward(saved, *masks, *logits)
        ctx.tcat = tcat                     # a constant of the step (no autograd history): kept alive for the backward
        ctx.cfg = (m, K1, masking, share, tdt, L, B, N, P)
        ctx.in_dtypes = [t.dtype for t in preds]
        ctx.in_shapes = [tuple(t.shape) for t in preds]
        return losses

    @staticmethod
    @once_differentiable
    def backward(ctx, d_losses):
        from .modules import _stream
        saved, *ts = ctx.saved_tensors
        m, K1, masking, share, tdt, L, B, N, P = ctx.cfg
        masks, logits = ts[:L], ts[L:]
        dev = saved.device
        g = f32c(d_losses)
        with torch.cuda.device(dev):
            need = ctx.needs_input_grad[7:]
            dm = [torch.empty_like(x) if need[i] else None for i, x in enumerate(masks)]
            dl = [torch.empty_like(x) if need[L + i] else None for i, x in enumerate(logits)]
            _lib.check(_lib.lib().axvs_set_criterion_bwd(g.data_ptr(), _ptrs(masks), _ptrs(logits), None if ctx.tcat is None else ctx.tcat.data_ptr(),
                                                         tdt, (C.c_int * B)(*m), L, B, N, K1, P, int(masking), int(share), saved.data_ptr(),
                                                         _ptrs(dm), _ptrs(dl), _stream(dev)), "axvs_set_criterion_bwd")
        grads = [None if d is None else d.reshape(s) for d, s in zip(dm + dl, ctx.in_shapes)]
        return (None,) * 7 + tuple(cast(grads, ctx.in_dtypes))


def _layers_of(outputs: Dict) -> List[Dict[str, Tensor]]:
    return [_final_layer(outputs)] + list(outputs.get("aux_outputs", []))


def _criterion(outputs: Dict, targets: List[Dict[str, Tensor]], num_classes: int, masking_void_pixel: bool, share_final_matching: bool,
               matched: Optional[Dict] = None, matcher_masking: Optional[bool] = None) -> Tensor:
    """-> losses [L, 3]; layer 0 = the final prediction, 1 + i = aux_outputs[i]"""
    layers = _layers_of(outputs)
    for o in layers:
        if not o["pred_masks"].is_cuda or not o["pred_logits"].is_cuda:
            raise RuntimeError(f"axial_vs_amd: pred_masks / pred_logits must be GPU tensors (got {o['pred_masks'].device}, "
                               f"{o['pred_logits'].device}); there is no CPU fallback")
    pm0, pl0 = layers[0]["pred_masks"], layers[0]["pred_logits"]
    B, N = pm0.shape[:2]
    P = pm0[0, 0].numel()
    K1 = pl0.shape[-1]
    if K1 != num_classes + 1:
        raise RuntimeError(f"pred_logits has {K1} channels for num_classes = {num_classes} (+ the void class)")
    for o in layers:
        if o["pred_masks"].shape != pm0.shape or o["pred_logits"].shape != pl0.shape:
            raise RuntimeError("every layer's pred_masks / pred_logits must have the final prediction's shape")
    # the predictions that are matched (cc_criterion.py:423-429, :442): the clip prediction or the final one, then every auxiliary layer
    # unless the final matching is shared.  16-bit predictions are matched and scored as fp32, as the models hand them over.
    first = _final_layer(matched) if matched is not None else layers[0]
    to_match = [first] + ([] if share_final_matching else layers[1:])
    to_match = [{"pred_masks": o["pred_masks"].detach().float(), "pred_logits": o["pred_logits"].detach().float()} for o in to_match]
    with _device_of(layers), torch.no_grad():
        m = [int(t["labels"].shape[0]) for t in targets]
        for t in targets:
            if not t["masks"].is_cuda or not t["labels"].is_cuda:
                raise RuntimeError(f"axial_vs_amd: target masks / labels must be GPU tensors (got {t['masks'].device}, {t['labels'].device}); "
                                   "there is no CPU fallback")
        if len(targets) != B:
            raise RuntimeError(f"{len(targets)} targets for a batch of {B}")
        cat = _cat_targets(targets, m, P, torch.float32) if max(m) > 0 else (None, None)
        _, _, _, rows, cols, dice, cls = _run_matcher(to_match, targets, masking_void_pixel if matcher_masking is None else matcher_masking,
                                                      cat=cat if max(m) > 0 else None)
    cfg = (m, int(rows.shape[1]), K1, bool(masking_void_pixel), bool(share_final_matching))
    with _device_of(layers):
        return _SetCriterion.apply(cfg, cat[0], cat[1], rows, cols, dice, cls, *[o["pred_masks"] for o in layers], *[o["pred_logits"] for o in layers])


def _as_dict(losses: Tensor, n_aux: int, names=("labels", "masks")) -> Dict[str, Tensor]:
    flat = losses.reshape(-1)          # (entries are selects, not an unbind: the models scale them in place, `losses[k] *= weight_dict[k]`)
    out = {}
    for l in range(1 + n_aux):
        for name in names:
            for k in LOSS_KEYS[name]:
                out[k if l == 0 else f"{k}_{l - 1}"] = flat[3 * l + _SLOT[k]]
    return out


def set_criterion_losses(outputs: Dict, targets: List[Dict[str, Tensor]], num_classes: int, masking_void_pixel: bool = True,
                         share_final_matching: bool = True) -> Dict[str, Tensor]:
    """The `labels` and `masks` losses of the final prediction and of every entry of outputs["aux_outputs"]: a dict of 0-dim fp32
    tensors in the reference's order (loss_ce, loss_mask, loss_dice, then the same with the suffix _{i} per auxiliary layer),
    differentiable with respect to every layer's pred_masks [B, N, T, H, W] and pred_logits [B, N, K + 1].  targets: per video
    {"labels": int64 [M_b], "masks": bool / uint8 / float [M_b, T, H, W]} on the GPU.  N <= 512, M_b <= 512; a label outside
    0 .. K-1 is clamped as the matcher does (the reference raises)."""
    losses = _criterion(outputs, targets, num_classes, masking_void_pixel, share_final_matching)
    return _as_dict(losses, len(outputs.get("aux_outputs", [])))


class MaXTronCCSetCriterion(nn.Module):
    """maxtron_deeplab/modeling/cc_criterion.py:203-453 with the reference's constructor, attributes, `forward(outputs, targets,
    clip_outputs=None)` and result keys; the `labels` and `masks` losses and their gradients run in libaxvs.so.

    `losses` may name "labels" and "masks" only: "pixels" and "aux_semantic" draw Gumbel noise (cc_criterion.py:59-65) and no shipped
    model requests them, so they raise here at construction instead of falling back to torch.  `matcher` is accepted and kept as an
    attribute; the call runs the library's matcher with that matcher's `masking_void_pixel` (the criterion's own when it has none).
    `eos_coef` and `weight_dict` are unused, as in the reference.  Inputs must be GPU tensors (no CPU fallback); a label outside
    0 .. K-1 is clamped as the matcher does, where the reference raises."""

    def __init__(self, num_classes, matcher, weight_dict, eos_coef, losses, share_final_matching, process_semantic=False,
                 pixel_insdis_temperature=1.5, pixel_insdis_sample_k=4096, aux_semantic_temperature=2.0, aux_semantic_sample_k=4096,
                 masking_void_pixel=True):
        super().__init__()
        for name in losses:
            if name not in LOSS_KEYS:
                raise NotImplementedError(f"axial_vs_amd: loss '{name}' is not built: the device criterion computes 'labels' and 'masks', the two "
                                          "every shipped model requests; 'pixels' and 'aux_semantic' sample pixels with Gumbel noise")
        self.num_classes = num_classes
        self.matcher = matcher
        self.weight_dict = weight_dict
        self.eos_coef = eos_coef
        self.losses = losses
        self.share_final_matching = share_final_matching
        self.process_semantic = process_semantic
        self.pixel_insdis_temperature = pixel_insdis_temperature
        self.pixel_insdis_sample_k = pixel_insdis_sample_k
        self.aux_semantic_temperature = aux_semantic_temperature
        self.aux_semantic_sample_k = aux_semantic_sample_k
        self.masking_void_pixel = masking_void_pixel

    def forward(self, outputs, targets, clip_outputs=None):
        mm = getattr(self.matcher, "masking_void_pixel", self.masking_void_pixel)
        losses = _criterion(outputs, targets, self.num_classes, self.masking_void_pixel, self.share_final_matching, matched=clip_outputs,
                            matcher_masking=mm)
        return _as_dict(losses, len(outputs.get("aux_outputs", [])), tuple(self.losses))

    def extra_repr(self) -> str:
        return (f"losses={self.losses}, num_classes={self.num_classes}, share_final_matching={self.share_final_matching}, "
                f"masking_void_pixel={self.masking_void_pixel}")


class MaXTronWCSetCriterion(MaXTronCCSetCriterion):
    """maxtron_deeplab/modeling/wc_criterion.py: the same criterion without `clip_outputs`."""

    def forward(self, outputs, targets):
        return super().forward(outputs, targets)
