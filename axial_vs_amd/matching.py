"""Matching on the device: clip-to-clip query alignment and prediction-to-ground-truth matching.

Reference: MaXTron_Video-kMaX/maxtron_deeplab/maxtron_cc_model.py:280-301 (the per-video loop that aligns every clip's
queries to the previous clip's) and :360-369 (`match_from_embds`: cosine cost + scipy.optimize.linear_sum_assignment on the
CPU); Tube-Link: models/video/tube_link_vis/mask2former_video_cc_head.py:907-913, :1038-1050.
`VideoHungarianMatcher`: maxtron_deeplab/modeling/matcher.py:48-124, called by cc_criterion.py:429,442 once for the final
prediction and once per auxiliary layer (softmax over the full [Q, T*H*W] mask logits, void-pixel multiply, einsum, `C.cpu()`,
SciPy: one host synchronisation per video per layer).
Here the cost matrices and the assignments run in libaxvs.so and the indices stay on the GPU: no `.cpu()` sync per clip pair,
per video or per layer.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence, Tuple

import torch
from torch import Tensor, nn

from . import _lib
from .modules import _dev_f32, _stream, _workspace, _guarded, _on, _select_status_word


@_guarded
def linear_sum_assignment(cost: Tensor, num_cols: Optional[Sequence[int]] = None):
    """scipy.optimize.linear_sum_assignment on the device (one wave per problem; sizes up to 512 on either side).

    Square cost fp32 [n,n] or [batch,n,n] (CUDA) -> int64 column index per row = SciPy's `col_ind` (its `row_ind` is arange(n)).
    Rectangular cost [n,m] or [batch,n,m], n != m -> (row_ind, col_ind), int64 on the device, min(n,m) pairs sorted by row: SciPy's pair.
    `num_cols` (host ints, one per problem, each <= m): problem z uses only its first num_cols[z] columns; always returns the pair,
    shaped [batch, min(n,m)] with the unused tail -1.
    Costs must be finite: SciPy raises on NaN / -inf entries, the kernel does not look at them (its result is then undefined)."""
    c = _dev_f32(cost, "cost")
    squeeze = c.dim() == 2
    if squeeze:
        c = c[None]
    if c.dim() != 3:
        raise RuntimeError(f"cost {tuple(cost.shape)} must be [n, m] or [batch, n, m]")
    b, n, m = c.shape
    if n == m and num_cols is None:
        out = torch.empty(b, n, dtype=torch.int64, device=c.device)
        _lib.check(_lib.lib().axvs_linear_sum_assignment(c.data_ptr(), out.data_ptr(), b, n, _stream(c.device)), "axvs_linear_sum_assignment")
        return out[0] if squeeze else out
    k = min(n, m)
    rows = torch.empty(b, k, dtype=torch.int64, device=c.device)
    cols = torch.empty(b, k, dtype=torch.int64, device=c.device)
    counts = None
    if num_cols is not None:
        if len(num_cols) != b:
            raise RuntimeError(f"num_cols has {len(num_cols)} entries for {b} problems")
        counts = (C.c_int * b)(*[int(x) for x in num_cols])
    if k > 0 and b > 0:
        _lib.check(_lib.lib().axvs_linear_sum_assignment_rect(c.data_ptr(), m, n, m, counts, rows.data_ptr(), cols.data_ptr(), b, _stream(c.device)),
                   "axvs_linear_sum_assignment_rect")
    return (rows[0], cols[0]) if squeeze else (rows, cols)


def _mask_dtype(t: Tensor) -> int:
    return {torch.float32: _lib.AXVS_F32, torch.float16: _lib.AXVS_F16, torch.bfloat16: _lib.AXVS_BF16}[t.dtype]


def _cat_targets(targets: List[Dict[str, Tensor]], m: List[int], P: int, mdt: torch.dtype) -> Tuple[Tensor, Tensor]:
    """The videos' ground truth concatenated along M, as the library takes it: masks [sum M_b, P] (uint8 for bool / uint8 targets,
    else fp32 through `mdt`) and int64 labels [sum M_b].  Videos without objects contribute nothing."""
    tm, tl = [], []
    for t, mb in zip(targets, m):
        gm, gl = t["masks"], t["labels"]
        if mb == 0:
            continue
        if gm.shape[0] != mb or gm[0].numel() != P:
            raise RuntimeError(f"target masks {tuple(gm.shape)} do not match {mb} labels and {P} predicted pixels")
        if gm.dtype == torch.bool:
            gm = gm.view(torch.uint8) if gm.is_contiguous() else gm.to(torch.uint8)
        elif gm.dtype != torch.uint8:
            gm = gm.to(mdt).float()            # matcher.py:81,83: `.to(out_mask)` then `.float()`
        tm.append(gm.flatten(1))
        tl.append(gl.to(torch.int64))
    if len({x.dtype for x in tm}) > 1:
        tm = [x.float() for x in tm]
    tcat = (tm[0] if len(tm) == 1 else torch.cat(tm)).contiguous()
    lcat = (tl[0] if len(tl) == 1 else torch.cat(tl)).contiguous()
    return tcat, lcat


def _run_matcher(layers: List[Dict[str, Tensor]], targets: List[Dict[str, Tensor]], masking_void_pixel: bool, cat=None):
    """All (layer, video) problems in one library call (`cat`: the caller's `_cat_targets` result, when it has one).  Returns (m, Q, sims [3, L*B, Q, M_max], rows, cols, dice, cls [L*B, min(Q, M_max)])."""
    masks, logits = [], []
    for o in layers:
        pm, pl = o["pred_masks"], o["pred_logits"]
        if not pm.is_cuda or not pl.is_cuda:
            raise RuntimeError(f"axial_vs_amd: pred_masks / pred_logits must be GPU tensors (got {pm.device}, {pl.device}); there is no CPU fallback")
        if pm.dtype not in (torch.float32, torch.float16, torch.bfloat16):
            pm = pm.float()
        masks.append(pm.flatten(2).contiguous())
        logits.append(pl.float().contiguous())
    dev, mdt = masks[0].device, masks[0].dtype
    B, Q, P = masks[0].shape
    K1 = logits[0].shape[-1]
    if len(targets) != B:
        raise RuntimeError(f"{len(targets)} targets for a batch of {B}")
    for pm, pl in zip(masks, logits):
        if pm.shape != (B, Q, P) or pm.dtype != mdt or pl.shape != (B, Q, K1):
            raise RuntimeError("every layer's pred_masks / pred_logits must have the final prediction's shape and dtype")
    for t in targets:
        if not t["masks"].is_cuda or not t["labels"].is_cuda:
            raise RuntimeError(f"axial_vs_amd: target masks / labels must be GPU tensors (got {t['masks'].device}, {t['labels'].device}); "
                               "there is no CPU fallback")
    m = [int(t["labels"].shape[0]) for t in targets]
    M_max, L = max(m), len(layers)
    k = min(Q, M_max)
    nprob = L * B
    rows = torch.empty(nprob, k, dtype=torch.int64, device=dev)
    cols = torch.empty(nprob, k, dtype=torch.int64, device=dev)
    dice = torch.empty(nprob, k, dtype=torch.float32, device=dev)
    cls = torch.empty(nprob, k, dtype=torch.float32, device=dev)
    sims = torch.empty(3, nprob, Q, M_max, dtype=torch.float32, device=dev)
    if M_max == 0:
        return m, Q, sims, rows, cols, dice, cls
    tcat, lcat = cat if cat is not None else _cat_targets(targets, m, P, mdt)
    Lb = _lib.lib()
    st = _stream(dev)
    ws = _workspace(dev, Lb.axvs_video_matcher_workspace_bytes(L, B, Q, M_max, P), st)
    _lib.check(Lb.axvs_video_matcher(_lib.ptrs(masks), _mask_dtype(masks[0]), _lib.ptrs(logits), tcat.data_ptr(),
                                     _lib.AXVS_U8 if tcat.dtype == torch.uint8 else _lib.AXVS_F32, lcat.data_ptr(), (C.c_int * B)(*m),
                                     L, B, Q, K1, P, M_max, int(bool(masking_void_pixel)), sims.data_ptr(), rows.data_ptr(), cols.data_ptr(),
                                     dice.data_ptr(), cls.data_ptr(), ws.data_ptr(), ws.numel(), st), "axvs_video_matcher")
    return m, Q, sims, rows, cols, dice, cls


def _layer_triples(n_layers: int, m: List[int], Q: int, rows: Tensor, cols: Tensor, dice: Tensor, cls: Tensor):
    B = len(m)
    out = []
    for l in range(n_layers):
        ks = [(l * B + b, min(Q, mb)) for b, mb in enumerate(m)]       # lengths are known on the host: slicing needs no sync
        out.append(([(rows[z, :k], cols[z, :k]) for z, k in ks], [dice[z, :k] for z, k in ks], [cls[z, :k] for z, k in ks]))
    return out


def _final_layer(outputs: Dict) -> Dict[str, Tensor]:
    return {k: v for k, v in outputs.items() if k != "aux_outputs"}


class _device_of:
    """the library launches on the current HIP device: make the predictions' device current around a call (what `_guarded` does for
    functions whose first argument is a tensor)"""

    def __init__(self, layers):
        t = layers[0]["pred_masks"]
        self.ctx = _on(t.device) if t.is_cuda else None
        self.dev = t.device

    def __enter__(self):
        if self.ctx is not None:
            self.ctx.__enter__()
            _select_status_word(self.dev)

    def __exit__(self, *exc):
        return self.ctx.__exit__(*exc) if self.ctx is not None else False


def _match(layers, targets, masking_void_pixel):
    with _device_of(layers):
        m, Q, _, rows, cols, dice, cls = _run_matcher(layers, targets, masking_void_pixel)
    return _layer_triples(len(layers), m, Q, rows, cols, dice, cls)


@torch.no_grad()
def match_layers(outputs: Dict, targets: List[Dict[str, Tensor]], masking_void_pixel: bool = True):
    """`VideoHungarianMatcher` for the final prediction AND every entry of outputs["aux_outputs"] in one batched library call
    (cc_criterion.py:429,442 calls the matcher once per layer).  Returns a list of the reference's triples
    (indices, matched_dice, matched_cls_prob): entry 0 for the final prediction, entry 1 + i for aux_outputs[i]."""
    return _match([_final_layer(outputs)] + list(outputs.get("aux_outputs", [])), targets, masking_void_pixel)


@torch.no_grad()
def matcher_costs(outputs: Dict[str, Tensor], targets: List[Dict[str, Tensor]], masking_void_pixel: bool = True):
    """The matcher's intermediate matrices per video: (mask_similarity, class_similarity, C = -mask_sim * class_sim), fp32 [Q, M_b]
    (matcher.py:78-86)."""
    layers = [_final_layer(outputs)]
    with _device_of(layers):
        m, Q, sims, *_ = _run_matcher(layers, targets, masking_void_pixel)
    return [tuple(sims[i, b, :, :mb] for i in range(3)) for b, mb in enumerate(m)]


class VideoHungarianMatcher(nn.Module):
    """maxtron_deeplab/modeling/matcher.py:48-124 with the reference's constructor and
    `forward(outputs, targets) -> (indices, matched_dice, matched_cls_prob)`: per video a tuple (row_ind, col_ind) of int64 tensors
    of length min(Q, M_b), and the mask / class similarity at the matched pairs (fp32, the same length).

    Unlike the reference, whose index tensors live on the CPU (they come out of SciPy), everything returned here stays ON THE
    GPU and the call does not synchronise with the host; `process_gt`'s indexing (cc_criterion.py:339-) works with device indices.
    Inputs must be GPU tensors (there is no CPU fallback).  Costs must be finite (SciPy raises on NaN / inf; here the result is
    undefined).  `match_layers` runs the final prediction and all auxiliary layers in one call."""

    def __init__(self, masking_void_pixel: bool = True):
        super().__init__()
        self.masking_void_pixel = masking_void_pixel

    @torch.no_grad()
    def forward(self, outputs, targets):
        return _match([_final_layer(outputs)], targets, self.masking_void_pixel)[0]

    def extra_repr(self) -> str:
        return f"masking_void_pixel={self.masking_void_pixel}"


@_guarded
def match_from_embds(tgt_embds: Tensor, cur_embds: Tensor) -> Tensor:
    """maxtron_cc_model.py:360-369: permutation (int64, on the device) that makes `cur_embds` align with `tgt_embds`."""
    t = _dev_f32(tgt_embds, "tgt_embds")
    c = _dev_f32(cur_embds, "cur_embds")
    if t.shape != c.shape or t.dim() != 2:
        raise RuntimeError(f"tgt_embds {tuple(t.shape)} and cur_embds {tuple(c.shape)} must be equal [Q, C] matrices")
    Q, Cc = t.shape
    L = _lib.lib()
    ws = _workspace(t.device, L.axvs_match_embds_workspace_bytes(Q, Cc))
    idx = torch.empty(Q, dtype=torch.int64, device=t.device)
    _lib.check(L.axvs_match_embds(t.data_ptr(), c.data_ptr(), idx.data_ptr(), Q, Cc, ws.data_ptr(), ws.numel(), _stream(t.device)),
               "axvs_match_embds")
    return idx


@_guarded
def match_clips(pred_mask_embeddings: Tensor, pred_cluster_centers: Tensor) -> Tensor:
    """maxtron_cc_model.py:280-301: per video, align the queries of clip i to the already aligned clip i-1 by their mask
    embeddings and carry the cluster centres along.  pred_mask_embeddings / pred_cluster_centers [B, Tc, Q, C*] ->
    matched cluster centres [B, Q, Tc, C] (the `clip_query` input of CrossClipTrackingModule)."""
    emb = _dev_f32(pred_mask_embeddings, "pred_mask_embeddings")
    cen = pred_cluster_centers
    B, Tc, Q, Cc = emb.shape
    if Tc == 1:
        return cen.permute(0, 2, 1, 3).contiguous()
    L = _lib.lib()
    ws = _workspace(emb.device, L.axvs_match_clips_workspace_bytes(B, Tc, Q, Cc))
    idx = torch.empty(B, Tc - 1, Q, dtype=torch.int64, device=emb.device)
    _lib.check(L.axvs_match_clips(emb.data_ptr(), idx.data_ptr(), B, Tc, Q, Cc, ws.data_ptr(), ws.numel(), _stream(emb.device)),
               "axvs_match_clips")
    # carry the cluster centres along: clip 0 as is, clip i permuted by its alignment (plumbing: one gather)
    aligned = torch.cat([cen[:, :1], torch.gather(cen[:, 1:], 2, idx[..., None].expand(-1, -1, -1, cen.shape[-1]))], dim=1)
    return aligned.permute(0, 2, 1, 3).contiguous()
