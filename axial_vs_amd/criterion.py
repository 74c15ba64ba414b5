"""The set criterion of the Video-kMaX models on the device: `MaXTronCCSetCriterion` / `MaXTronWCSetCriterion`.

Reference: MaXTron_Video-kMaX/maxtron_deeplab/modeling/cc_criterion.py:203-453 (wc_criterion.py is the same class without
`clip_outputs`).  There, every layer scatters the ground truth into a zero tensor shaped like pred_masks, takes a softmax over the
queries for the void IoU, again for the dice term, a log-softmax for the mask cross-entropy, and autograd keeps those maps.  Here the
matcher's indices stay on the GPU (matching.py), the `labels` and `masks` losses of ALL layers come out of one library call that reads
pred_masks once, the backward reads it once more and writes the gradient once, and what is kept in between is O(L * B * N).  No
[B, N, P] temporary exists besides the gradient, and the host is never synchronised.

The `'pixels'` and `'aux_semantic'` losses (wc_criterion.py:62-142, :271-305) are what every within-clip config adds
(INSDIS_WEIGHT / AUX_SEMANTIC_WEIGHT 1.0, maxtron_wc_model.py:130-134): a Gumbel top-k sample of k of the P pixels per (prediction,
video), the pixel-wise instance-discrimination loss over the K x K similarities of the sampled pixel features, and a cross-entropy
of the auxiliary semantic prediction at its own samples.  `MaXTronWCSetCriterion` computes them in the library too
(`sampled_pixel_losses`): the keys come from the matcher's pairs and the concatenated targets the `labels` / `masks` call already
has, the k largest keys of a row are picked by a radix select, the K x K matrices are streamed through the f32-input MFMA tile by
tile and never stored, and O(L * B * k) statistics are kept for the backward.  The uniform noise is drawn with `torch.rand` in the
reference's call order (`draw_sampling_noise`), so a seeded step samples the pixels the reference samples.  The cross-clip criterion
(maxtron_cc_model.py:147 hard-codes ["labels", "masks"]) keeps refusing the two names at construction.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence, Tuple

import torch
from torch import Tensor, nn
from torch.autograd.function import once_differentiable

from . import _lib
from ._autograd import cast, f32c, nbytes, place, require_gpu
from .matching import _cat_targets, _device_of, _final_layer, _run_matcher

LOSS_KEYS = {"labels": ("loss_ce",), "masks": ("loss_mask", "loss_dice")}
SAMPLED_LOSS_KEYS = {"pixels": ("loss_pixel_insdis",), "aux_semantic": ("loss_aux_semantic",)}      # the within-clip criterion's two more
MAX_SAMPLE_K, MAX_FEATURE_CHANNELS, MAX_PIXELS = 8192, 256, 1 << 20                                # include/axvs.h, axvs_pixel_*
_SLOT = {"loss_ce": 0, "loss_mask": 1, "loss_dice": 2}


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
            _lib.check(lib.axvs_set_criterion_fwd(_lib.ptrs(masks), _lib.ptrs(logits), None if tcat is None else tcat.data_ptr(), tdt,
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
            _lib.check(_lib.lib().axvs_set_criterion_bwd(g.data_ptr(), _lib.ptrs(masks), _lib.ptrs(logits), None if ctx.tcat is None else ctx.tcat.data_ptr(),
                                                         tdt, (C.c_int * B)(*m), L, B, N, K1, P, int(masking), int(share), saved.data_ptr(),
                                                         _lib.ptrs(dm), _lib.ptrs(dl), _stream(dev)), "axvs_set_criterion_bwd")
        grads = [None if d is None else d.reshape(s) for d, s in zip(dm + dl, ctx.in_shapes)]
        return (None,) * 7 + tuple(cast(grads, ctx.in_dtypes))


def _layers_of(outputs: Dict) -> List[Dict[str, Tensor]]:
    return [_final_layer(outputs)] + list(outputs.get("aux_outputs", []))


class _Step:
    """What one criterion call knows after matching: the layers, the concatenated targets and the matcher's result (all on the GPU)."""
    __slots__ = ("layers", "m", "B", "N", "P", "K1", "cat", "rows", "cols", "dice", "cls", "share")


def _match_step(outputs: Dict, targets: List[Dict[str, Tensor]], num_classes: int, masking_void_pixel: bool, share_final_matching: bool,
                matched: Optional[Dict] = None, matcher_masking: Optional[bool] = None) -> _Step:
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
    st = _Step()
    st.layers, st.m, st.B, st.N, st.P, st.K1, st.cat, st.share = layers, m, B, N, P, K1, cat, bool(share_final_matching)
    st.rows, st.cols, st.dice, st.cls = rows, cols, dice, cls
    return st


def _set_losses(st: _Step, masking_void_pixel: bool) -> Tensor:
    """-> losses [L, 3]; layer 0 = the final prediction, 1 + i = aux_outputs[i]"""
    cfg = (st.m, int(st.rows.shape[1]), st.K1, bool(masking_void_pixel), st.share)
    with _device_of(st.layers):
        return _SetCriterion.apply(cfg, st.cat[0], st.cat[1], st.rows, st.cols, st.dice, st.cls, *[o["pred_masks"] for o in st.layers],
                                   *[o["pred_logits"] for o in st.layers])


def _criterion(outputs: Dict, targets: List[Dict[str, Tensor]], num_classes: int, masking_void_pixel: bool, share_final_matching: bool,
               matched: Optional[Dict] = None, matcher_masking: Optional[bool] = None) -> Tensor:
    return _set_losses(_match_step(outputs, targets, num_classes, masking_void_pixel, share_final_matching, matched, matcher_masking),
                       masking_void_pixel)


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


# ---- the sampled pixel losses of the within-clip criterion ---------------------------------------------------------------------------
def draw_sampling_noise(n_layers: int, B: int, P: int, pixels: bool, aux_semantic: bool, device, generator=None,
                        semantic_first: bool = False) -> Tuple[Optional[Tensor], Optional[Tensor]]:
    """The uniform noise of one criterion call, drawn as the reference's `forward` draws it (wc_criterion.py:65, :434-450): one
    `torch.rand((B, P))` fp32 per call of `_gumbel_topk_sample`, for the final prediction's `pixels`, then its `aux_semantic`, then
    the `pixels` of aux_outputs[0], [1], ...  -> (u_pixels [n_layers, B, P] or None, u_semantic [B, P] or None).  Under the same seed
    this consumes `generator` (default: the device's) exactly as the reference does.  `semantic_first`: the `losses` list names
    "aux_semantic" before "pixels" (the reference draws in list order)."""
    def rand():
        return torch.rand((B, P), dtype=torch.float32, device=device, generator=generator)
    up: List[Tensor] = []
    us = None
    if aux_semantic and semantic_first:
        us = rand()
    if pixels:
        up.append(rand())
    if aux_semantic and not semantic_first:
        us = rand()
    if pixels:
        up += [rand() for _ in range(n_layers - 1)]
    return (torch.stack(up) if pixels else None), us


class _PixelInsdis(torch.autograd.Function):
    """losses [L] (loss_pixel_insdis per layer) of L layers' pixel_feature [B, C, P] at the sampled pixels idx [L, B, k]."""

    @staticmethod
    def forward(ctx, cfg, tcat, cols, idx, *feats):
        from .modules import _stream
        m, kmax, N, share, k = cfg
        for t in feats:
            require_gpu(t)
        fs = [f32c(t).flatten(2) for t in feats]
        dev = fs[0].device
        L, (B, Cf, P) = len(fs), fs[0].shape
        lib = _lib.lib()
        tdt = _lib.AXVS_F32 if (tcat is not None and tcat.dtype == torch.float32) else _lib.AXVS_U8
        with torch.cuda.device(dev):
            losses = torch.empty(L, dtype=torch.float32, device=dev)
            saved, saved_ptr, scratch = place(dev, nbytes("axvs_pixel_insdis_saved_bytes", L, B, k),
                                              nbytes("axvs_pixel_insdis_workspace_bytes", L, B, Cf, kmax, k))
            _lib.check(lib.axvs_pixel_insdis_fwd(_lib.ptrs(fs), None if tcat is None else tcat.data_ptr(), tdt, (C.c_int * B)(*m),
                                                 None if kmax == 0 else cols.data_ptr(), kmax, int(share), L, B, N, Cf, P, idx.data_ptr(), k,
                                                 int(idx.shape[-1]), losses.data_ptr(), saved_ptr, scratch.data_ptr(), scratch.numel(),
                                                 _stream(dev)), "axvs_pixel_insdis_fwd")
        ctx.save_for_backward(saved, idx, *fs)
        ctx.tcat, ctx.cols = tcat, cols          # constants of the step (no autograd history): kept alive for the backward
        ctx.cfg = (m, kmax, N, share, k, tdt, L, B, Cf, P)
        ctx.in_dtypes = [t.dtype for t in feats]
        ctx.in_shapes = [tuple(t.shape) for t in feats]
        return losses

    @staticmethod
    @once_differentiable
    def backward(ctx, d_losses):
        from .modules import _stream, _workspace
        saved, idx, *fs = ctx.saved_tensors
        m, kmax, N, share, k, tdt, L, B, Cf, P = ctx.cfg
        dev = saved.device
        g = f32c(d_losses)
        with torch.cuda.device(dev):
            need = ctx.needs_input_grad[4:]
            df = [torch.zeros_like(x) if need[i] else None for i, x in enumerate(fs)]       # only the sampled pixels are written
            scratch = _workspace(dev, nbytes("axvs_pixel_insdis_workspace_bytes", L, B, Cf, kmax, k))
            _lib.check(_lib.lib().axvs_pixel_insdis_bwd(g.data_ptr(), _lib.ptrs(fs), None if ctx.tcat is None else ctx.tcat.data_ptr(), tdt,
                                                        (C.c_int * B)(*m), None if kmax == 0 else ctx.cols.data_ptr(), kmax, int(share), L, B, N,
                                                        Cf, P, idx.data_ptr(), k, int(idx.shape[-1]), saved.data_ptr(), _lib.ptrs(df),
                                                        scratch.data_ptr(), scratch.numel(), _stream(dev)), "axvs_pixel_insdis_bwd")
        grads = [None if d is None else d.reshape(s) for d, s in zip(df, ctx.in_shapes)]
        return (None,) * 4 + tuple(cast(grads, ctx.in_dtypes))


class _AuxSemantic(torch.autograd.Function):
    """loss [1] (loss_aux_semantic) of aux_semantic_pred [B, Cs, P] against sem int64 [B, P] at the sampled pixels idx [B, k]."""

    @staticmethod
    def forward(ctx, cfg, sem, idx, pred):
        from .modules import _stream
        num_classes, k = cfg
        require_gpu(pred)
        x = f32c(pred).flatten(2)
        dev = x.device
        B, Cs, P = x.shape
        with torch.cuda.device(dev):
            loss = torch.empty(1, dtype=torch.float32, device=dev)
            saved = torch.empty(nbytes("axvs_pixel_semantic_saved_bytes", B, k), dtype=torch.uint8, device=dev)
            _lib.check(_lib.lib().axvs_pixel_semantic_fwd(x.data_ptr(), sem.data_ptr(), idx.data_ptr(), k, int(idx.shape[-1]), B, Cs, P,
                                                          num_classes, loss.data_ptr(), saved.data_ptr(), _stream(dev)), "axvs_pixel_semantic_fwd")
        ctx.save_for_backward(saved, idx, sem, x)
        ctx.cfg = (num_classes, k, B, Cs, P)
        ctx.in_dtype, ctx.in_shape = pred.dtype, tuple(pred.shape)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, d_loss):
        from .modules import _stream
        saved, idx, sem, x = ctx.saved_tensors
        num_classes, k, B, Cs, P = ctx.cfg
        g = f32c(d_loss)
        with torch.cuda.device(x.device):
            dx = torch.zeros_like(x)                                                       # only the sampled pixels are written
            _lib.check(_lib.lib().axvs_pixel_semantic_bwd(g.data_ptr(), x.data_ptr(), sem.data_ptr(), idx.data_ptr(), k, int(idx.shape[-1]), B, Cs,
                                                          P, num_classes, saved.data_ptr(), dx.data_ptr(), _stream(x.device)),
                       "axvs_pixel_semantic_bwd")
        return None, None, None, dx.reshape(ctx.in_shape).to(ctx.in_dtype)


def _check_sample_k(name: str, k, P: int) -> int:
    k = int(k)
    if k < 0 or k > MAX_SAMPLE_K:
        raise RuntimeError(f"axial_vs_amd: {name} = {k} is outside 0..{MAX_SAMPLE_K}")
    if k > P:
        raise RuntimeError(f"axial_vs_amd: {name} = {k} samples out of {P} pixels: selected index k out of range")
    return k


def _sampled_losses(st: _Step, targets, num_classes: int, names: Sequence[str], temperatures, ks, noise, generator, return_samples: bool):
    """The `pixels` / `aux_semantic` losses on the matching of `st` -> ({"pixels": [L] tensor, "aux_semantic": [1] tensor}, samples)"""
    from .modules import _stream
    pixels, semantic = "pixels" in names, "aux_semantic" in names
    layers, B, P, L = st.layers, st.B, st.P, len(st.layers)
    dev = layers[0]["pred_masks"].device
    if P > MAX_PIXELS:
        raise RuntimeError(f"axial_vs_amd: P = T*H*W = {P} pixels is above {MAX_PIXELS}")
    k_pix = _check_sample_k("pixel_insdis_sample_k", ks[0], P) if pixels else 0
    k_sem = _check_sample_k("aux_semantic_sample_k", ks[1], P) if semantic else 0
    feats, pred, sem = [], None, None
    if pixels:
        for i, o in enumerate(layers):
            if "pixel_feature" not in o:
                raise RuntimeError(f"axial_vs_amd: the 'pixels' loss needs outputs['pixel_feature'] of every prediction (missing in layer {i})")
            f = o["pixel_feature"]
            if not f.is_cuda:
                raise RuntimeError(f"axial_vs_amd: pixel_feature must be a GPU tensor (got {f.device}); there is no CPU fallback")
            if f.shape[0] != B or f[0, 0].numel() != P or f.shape[1:] != layers[0]["pixel_feature"].shape[1:]:
                raise RuntimeError(f"pixel_feature {tuple(f.shape)} of layer {i} does not match {B} videos of {P} pixels")
            if f.shape[1] % 4 or f.shape[1] > MAX_FEATURE_CHANNELS:
                raise RuntimeError(f"axial_vs_amd: pixel_feature has {f.shape[1]} channels: a multiple of 4 up to {MAX_FEATURE_CHANNELS} is needed")
            feats.append(f)
    if semantic:
        if "aux_semantic_pred" not in layers[0]:
            raise RuntimeError("axial_vs_amd: the 'aux_semantic' loss needs outputs['aux_semantic_pred']")
        pred = layers[0]["aux_semantic_pred"]
        if not pred.is_cuda:
            raise RuntimeError(f"axial_vs_amd: aux_semantic_pred must be a GPU tensor (got {pred.device}); there is no CPU fallback")
        if pred.shape[0] != B or pred[0, 0].numel() != P:
            raise RuntimeError(f"aux_semantic_pred {tuple(pred.shape)} does not match {B} videos of {P} pixels")
        if pred.shape[1] > MAX_FEATURE_CHANNELS:
            raise RuntimeError(f"axial_vs_amd: aux_semantic_pred has {pred.shape[1]} class channels: at most {MAX_FEATURE_CHANNELS}")
        for t in targets:
            if "semantic_masks" not in t:
                raise RuntimeError("axial_vs_amd: the 'aux_semantic' loss needs targets[b]['semantic_masks'] (process_semantic)")
            if not t["semantic_masks"].is_cuda or t["semantic_masks"].numel() != P:
                raise RuntimeError(f"semantic_masks must be a GPU tensor of {P} pixels (got {t['semantic_masks'].device}, "
                                   f"{tuple(t['semantic_masks'].shape)}); there is no CPU fallback")
        sem = torch.stack([t["semantic_masks"].reshape(P) for t in targets]).to(torch.int64).contiguous()
    if noise is None:
        order = [n for n in names if n in SAMPLED_LOSS_KEYS]
        noise = draw_sampling_noise(L, B, P, pixels, semantic, dev, generator, semantic_first=order[0] == "aux_semantic" and pixels)
    u_pix, u_sem = noise
    rows: List[Tuple[Tensor, int, float, int]] = []           # (noise [B, P], matching, temperature, k)
    if pixels:
        if u_pix is None or tuple(u_pix.shape) != (L, B, P):
            raise RuntimeError(f"noise[0] must be [{L}, {B}, {P}] uniform numbers for the 'pixels' loss")
        rows += [(f32c(u_pix[l]), 0 if st.share else l, float(temperatures[0]), k_pix) for l in range(L)]
    if semantic:
        if u_sem is None or tuple(u_sem.shape) != (B, P):
            raise RuntimeError(f"noise[1] must be [{B}, {P}] uniform numbers for the 'aux_semantic' loss")
        rows.append((f32c(u_sem), 0, float(temperatures[1]), k_sem))
    for u, *_ in rows:
        if not u.is_cuda:
            raise RuntimeError(f"axial_vs_amd: the sampling noise must be a GPU tensor (got {u.device}); there is no CPU fallback")
    R, kmax, LM = len(rows), int(st.rows.shape[1]), 1 if st.share else L
    kstride = max(1, k_pix, k_sem)
    tcat = st.cat[0]
    tdt = _lib.AXVS_F32 if (tcat is not None and tcat.dtype == torch.float32) else _lib.AXVS_U8
    with _device_of(layers), torch.no_grad():
        idx = torch.zeros(R, B, kstride, dtype=torch.int32, device=dev)
        keys = torch.empty(R, B, P, dtype=torch.float32, device=dev)
        area = torch.empty(max(1, LM * B * kmax), dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().axvs_pixel_sample(None if tcat is None else tcat.data_ptr(), tdt, (C.c_int * B)(*st.m),
                                                None if kmax == 0 else st.cols.data_ptr(), kmax, LM, B, st.N, P, _lib.ptrs([r[0] for r in rows]),
                                                (C.c_int * R)(*[r[1] for r in rows]), (C.c_float * R)(*[r[2] for r in rows]),
                                                (C.c_int * R)(*[r[3] for r in rows]), R, area.data_ptr(), keys.data_ptr(), idx.data_ptr(),
                                                kstride, _stream(dev)), "axvs_pixel_sample")
    out = {}
    with _device_of(layers):
        if pixels:
            out["pixels"] = _PixelInsdis.apply((st.m, kmax, st.N, st.share, k_pix), tcat, st.cols, idx[:L], *feats)
        if semantic:
            out["aux_semantic"] = _AuxSemantic.apply((int(num_classes), k_sem), sem, idx[R - 1], pred)
    samples = None
    if return_samples:
        samples = {"pixels": idx[:L, :, :k_pix] if pixels else None, "aux_semantic": idx[R - 1, :, :k_sem] if semantic else None,
                   "keys_pixels": keys[:L] if pixels else None, "keys_aux_semantic": keys[R - 1] if semantic else None}
    return out, samples


def _sampled_dict(res: Dict[str, Tensor], l: int, names) -> Dict[str, Tensor]:
    """layer l's entries of the sampled losses, in the order of `names` (aux_semantic: the final prediction only)"""
    out = {}
    for name in names:
        if name == "pixels":
            out["loss_pixel_insdis" if l == 0 else f"loss_pixel_insdis_{l - 1}"] = res["pixels"][l]
        elif name == "aux_semantic" and l == 0:
            out["loss_aux_semantic"] = res["aux_semantic"][0]
    return out


def sampled_pixel_losses(outputs: Dict, targets: List[Dict[str, Tensor]], num_classes: int, losses: Sequence[str] = ("pixels", "aux_semantic"),
                         share_final_matching: bool = True, masking_void_pixel: bool = True, pixel_insdis_temperature: float = 1.5,
                         pixel_insdis_sample_k: int = 4096, aux_semantic_temperature: float = 2.0, aux_semantic_sample_k: int = 4096,
                         noise=None, generator=None, return_samples: bool = False):
    """The `pixels` and `aux_semantic` losses of the within-clip criterion (wc_criterion.py:62-142, :271-305): a dict of 0-dim fp32
    tensors with the reference's keys (loss_pixel_insdis, loss_aux_semantic, then loss_pixel_insdis_{i} per auxiliary layer),
    differentiable with respect to every layer's pixel_feature [B, C, T, H, W] and to aux_semantic_pred [B, Cs, T, H, W].  The
    matching is the library's, on pred_masks / pred_logits as in `set_criterion_losses`; targets carry "semantic_masks" int [T, H, W]
    (-1: ignored) for `aux_semantic`.  `noise`: (u_pixels [L, B, P], u_semantic [B, P]) as `draw_sampling_noise` gives it; None draws
    it from `generator` (default: the device's) in the reference's order.  `return_samples`: also return the sampled pixel indices
    (int32, increasing per row; equal keys go to the lower pixel) and the fp32 keys.  C a multiple of 4 up to 256, Cs <= 256,
    k <= min(8192, P), P <= 2^20; anything else raises.  k = 0 gives a loss of exactly 0."""
    for name in losses:
        if name not in SAMPLED_LOSS_KEYS:
            raise ValueError(f"sampled_pixel_losses computes 'pixels' and 'aux_semantic', not '{name}'")
    st = _match_step(outputs, targets, num_classes, masking_void_pixel, share_final_matching)
    res, samples = _sampled_losses(st, targets, num_classes, tuple(losses), (pixel_insdis_temperature, aux_semantic_temperature),
                                   (pixel_insdis_sample_k, aux_semantic_sample_k), noise, generator, return_samples)
    out = {}
    for l in range(len(st.layers)):
        out.update(_sampled_dict(res, l, losses))
    return (out, samples) if return_samples else out


class MaXTronCCSetCriterion(nn.Module):
    """maxtron_deeplab/modeling/cc_criterion.py:203-453 with the reference's constructor, attributes, `forward(outputs, targets,
    clip_outputs=None)` and result keys; the `labels` and `masks` losses and their gradients run in libaxvs.so.

    `losses` may name "labels" and "masks" only: "pixels" and "aux_semantic" draw Gumbel noise (cc_criterion.py:59-65) and no
    cross-clip model requests them (maxtron_cc_model.py:147), so they raise here at construction instead of falling back to torch;
    `MaXTronWCSetCriterion` computes them.  `matcher` is accepted and kept as an
    attribute; the call runs the library's matcher with that matcher's `masking_void_pixel` (the criterion's own when it has none).
    `eos_coef` and `weight_dict` are unused, as in the reference.  Inputs must be GPU tensors (no CPU fallback); a label outside
    0 .. K-1 is clamped as the matcher does, where the reference raises."""

    _LOSSES = LOSS_KEYS      # the loss names this class takes

    def __init__(self, num_classes, matcher, weight_dict, eos_coef, losses, share_final_matching, process_semantic=False,
                 pixel_insdis_temperature=1.5, pixel_insdis_sample_k=4096, aux_semantic_temperature=2.0, aux_semantic_sample_k=4096,
                 masking_void_pixel=True):
        super().__init__()
        for name in losses:
            if name in self._LOSSES:
                continue
            if name in SAMPLED_LOSS_KEYS:
                raise NotImplementedError(f"axial_vs_amd: loss '{name}' is not built for the cross-clip criterion: no cross-clip model requests "
                                          "it (maxtron_cc_model.py:147); 'pixels' and 'aux_semantic' sample pixels with Gumbel noise and are "
                                          "computed by MaXTronWCSetCriterion")
            raise NotImplementedError(f"axial_vs_amd: there is no loss '{name}' (the reference has 'labels', 'masks', 'pixels', 'aux_semantic')")
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
    """maxtron_deeplab/modeling/wc_criterion.py:206-451: the same criterion without `clip_outputs`, with all four losses of the
    within-clip configs: "labels", "masks", "pixels" (`loss_pixel_insdis` of every prediction, from outputs["pixel_feature"]) and
    "aux_semantic" (`loss_aux_semantic` of the final prediction, from outputs["aux_semantic_pred"] and targets[b]["semantic_masks"];
    needs `process_semantic=True` as in the reference).  The result has the reference's keys in its order.  The matcher runs once for
    all four; the sampling noise comes from the default generator of the predictions' device through `draw_sampling_noise`, so a
    seeded call samples the reference's pixels.  See `sampled_pixel_losses` for the bounds."""

    _LOSSES = {**LOSS_KEYS, **SAMPLED_LOSS_KEYS}

    def forward(self, outputs, targets):
        names = tuple(self.losses)
        sampled = tuple(n for n in names if n in SAMPLED_LOSS_KEYS)
        if not sampled:
            return super().forward(outputs, targets)
        if "aux_semantic" in sampled and not self.process_semantic:
            raise RuntimeError("axial_vs_amd: the 'aux_semantic' loss needs process_semantic=True (wc_criterion.py:407-413 builds its ground "
                               "truth only then)")
        mm = getattr(self.matcher, "masking_void_pixel", self.masking_void_pixel)
        st = _match_step(outputs, targets, self.num_classes, self.masking_void_pixel, self.share_final_matching, matcher_masking=mm)
        flat = _set_losses(st, self.masking_void_pixel).reshape(-1) if any(n in LOSS_KEYS for n in names) else None
        res, _ = _sampled_losses(st, targets, self.num_classes, names, (self.pixel_insdis_temperature, self.aux_semantic_temperature),
                                 (self.pixel_insdis_sample_k, self.aux_semantic_sample_k), None, None, False)
        out = {}
        for l in range(len(st.layers)):
            for name in names:
                if name in LOSS_KEYS:
                    for k in LOSS_KEYS[name]:
                        out[k if l == 0 else f"{k}_{l - 1}"] = flat[3 * l + _SLOT[k]]
                else:
                    out.update(_sampled_dict(res, l, (name,)))
        return out
