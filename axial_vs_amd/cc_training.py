"""Training path of CrossClipTrackingModule: autograd over libaxvs.so's cross-clip training tier.

Reference: ``CrossClipTrackingModule.forward`` in ``train()`` mode under autograd, CC = MaXTron_Video-kMaX/maxtron_deeplab/modeling/
cross_clip_tracking_module/maxtron_cross_clip_tracking_module.py:275-322 with the predictor's training branch (:45-57) -- the module the
reference trains on its own with backbone and segmentation head frozen (maxtron_cc_model.py:104-108).  Forward and backward both run in
the library (``axvs_cc_module_train_fwd`` / ``_bwd``, include/axvs.h); this file is the ``torch.autograd.Function`` that binds them, the
running-statistics update of the four BatchNorm sites (momentum arithmetic on [C] vectors) and the SyncBatchNorm all-reduce callback.

* (Sync)BatchNorm: in ``train()`` mode the four ``ConvBN(norm='syncbn')`` sites normalise with BATCH statistics.  When
  ``torch.distributed`` is initialised with more than one rank the library's partial sums are summed over the ranks (RCCL
  all-reduce of 2 C + 1 floats per site and layer, three calls per forward and three per backward), as ``nn.SyncBatchNorm`` does.
* dropout masks are the same counter-based hash as the layer's training tier (sites 10 + 2 l: attention maps of layer l, 11 + 2 l:
  ASPP ``_proj_drop``); ``seed`` from torch's CPU generator or ``module.dropout_seed``.
* no gradient is produced for ``panoptic_features`` (the frozen segmenter's pixel features).

Tube-Link's ``TubeLinkCrossClipHead`` trains through two calls: the layer chain alone (``cc_layers_train``, ``axvs_cc_layers_train_*``)
and the prediction heads of all layers at once (``tl_heads_train``, ``axvs_tl_heads_train_*``: post_norm, class pooling, cls_embed, the
mask MLP, the per-clip mask einsum); its ``mask_features`` get a gradient when they ask for one.
"""
from __future__ import annotations

import ctypes as C
from typing import List

import torch
import torch.distributed as dist
from torch import Tensor

from . import _lib
from ._autograd import apply, cast, draw_seed, f32c, grad_buffer, nbytes, place, require_gpu
from ._params import CC_PER_LAYER as _PER_LAYER, cc_bn_modules, cc_chain_params, cc_head_with_running, cc_layer_struct, cc_module_params, tl_head_params


# the parameter lists handed to autograd (their names here are part of the tested surface): the chain's 21 tensors per layer, then the
# 15 of the heads; the Tube-Link head's 12 in AxvsTLHeadParams field order
chain_parameters = cc_chain_params
module_parameters = cc_module_params
tl_heads_parameters = tl_head_params


def _layers(ptrs: List[int], nl: int):
    """The AxvsCCLayerParams (or AxvsCCLayerGrads) array of `nl` layers from the chain's tensors."""
    return (_lib.AxvsCCLayerParams * nl)(*[cc_layer_struct(ptrs[i * _PER_LAYER:(i + 1) * _PER_LAYER]) for i in range(nl)])


def _head_struct(ptrs: List[int], running) -> _lib.AxvsCCHeadParams:
    return _lib.fill(_lib.AxvsCCHeadParams, cc_head_with_running(ptrs, running))


class _AllReduce:
    """The library's SyncBatchNorm hook: sums `n` floats at a device address inside `buf` over the ranks of `group`."""

    def __init__(self, buf: Tensor, group):
        self.buf, self.group, self.error = buf, group, None
        self.fn = _lib.ALLREDUCE_FN(self._call)

    def _call(self, user, ptr, n, stream):
        try:
            off = int(ptr) - self.buf.data_ptr()
            if off < 0 or off + 4 * n > self.buf.numel():
                raise RuntimeError("all-reduce buffer outside the scratch tensor")
            dist.all_reduce(self.buf[off:off + 4 * n].view(torch.float32), group=self.group)
            return 0
        except Exception as e:   # an exception may not cross the C frame
            self.error = e
            return 1


def _cfg(dims, rates, p_attn, p_aspp, seed, hook) -> _lib.AxvsCCTrainCfg:
    B, Q, Tc, V, H, W, K1, nl = dims
    c = _lib.AxvsCCTrainCfg()
    c.B, c.Q, c.Tc, c.V, c.H, c.W, c.K1, c.num_layers = B, Q, Tc, V, H, W, K1, nl
    for k in range(3):
        c.rates[k] = int(rates[k])
    c.p_attn_drop, c.p_aspp_drop, c.seed = float(p_attn), float(p_aspp), int(seed)
    c.allreduce = hook.fn if hook is not None else _lib.ALLREDUCE_FN()
    c.allreduce_user = None
    c.chain_only = 0
    return c


def _sync_group():
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        return dist.group.WORLD
    return None


class _CCModuleTrain(torch.autograd.Function):
    @staticmethod
    def forward(ctx, clip_query, panoptic_features, cfg, running, *params):
        from .modules import _stream
        dims, rates, p_attn, p_aspp, seed = cfg
        require_gpu(clip_query)
        B, Q, Tc, V, H, W, K1, nl = dims
        cq, pf = f32c(clip_query), f32c(panoptic_features)
        ws = [f32c(w) for w in params]
        rn = [(f32c(m), f32c(v)) for m, v in running]
        dev = cq.device
        group = _sync_group()
        with torch.cuda.device(dev):
            probe = _cfg(dims, rates, p_attn, p_aspp, seed, None)
            nsaved = nbytes("axvs_cc_module_train_saved_bytes", C.byref(probe))
            nscr = nbytes("axvs_cc_module_train_scratch_bytes", C.byref(probe), 0)
            nstat = _lib.lib().axvs_cc_module_train_bn_stats_floats(C.byref(probe))
            saved, _, scratch = place(dev, nsaved, nscr, shared=False)       # (the SyncBatchNorm hook checks its buffers lie in `scratch`)
            logits = torch.empty(nl, 1, Q, K1, dtype=torch.float32, device=dev)
            masks = torch.empty(nl, B, Q, Tc * V, H, W, dtype=torch.float32, device=dev)
            stats = torch.empty(nstat, dtype=torch.float32, device=dev)
            hook = _AllReduce(scratch, group) if group is not None else None
            c = _cfg(dims, rates, p_attn, p_aspp, seed, hook)
            ptrs = [w.data_ptr() for w in ws]
            heads = _head_struct(ptrs[nl * _PER_LAYER:], [(m.data_ptr(), v.data_ptr()) for m, v in rn])
            rc = _lib.lib().axvs_cc_module_train_fwd(cq.data_ptr(), pf.data_ptr(), logits.data_ptr(), masks.data_ptr(), stats.data_ptr(),
                                                     _layers(ptrs, nl), C.byref(heads), C.byref(c), saved.data_ptr(), nsaved,
                                                     scratch.data_ptr(), nscr, _stream(dev))
            if hook is not None and hook.error is not None:
                raise hook.error
            _lib.check(rc, "axvs_cc_module_train_fwd")
        ctx.save_for_backward(cq, pf, *ws)
        ctx.amp = _lib.current_amp()
        ctx.running = rn
        ctx.cfg = cfg
        ctx.saved_buf = saved
        ctx.in_dtypes = [t.dtype for t in (clip_query, *params)]
        ctx.mark_non_differentiable(stats)
        return logits, masks, stats

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_logits, d_masks, _d_stats):
        from .modules import _stream
        cq, pf, *ws = ctx.saved_tensors
        dims, rates, p_attn, p_aspp, seed = ctx.cfg
        B, Q, Tc, V, H, W, K1, nl = dims
        dev = cq.device
        group = _sync_group()
        with torch.cuda.device(dev):
            gl = f32c(d_logits) if d_logits is not None else torch.zeros(nl, 1, Q, K1, dtype=torch.float32, device=dev)
            gm = f32c(d_masks) if d_masks is not None else torch.zeros(nl, B, Q, Tc * V, H, W, dtype=torch.float32, device=dev)
            probe = _cfg(dims, rates, p_attn, p_aspp, seed, None)
            nsaved = nbytes("axvs_cc_module_train_saved_bytes", C.byref(probe))
            nscr = nbytes("axvs_cc_module_train_scratch_bytes", C.byref(probe), 1)
            _, saved_ptr, scratch = place(dev, nsaved, nscr, shared=False, saved=ctx.saved_buf)
            hook = _AllReduce(scratch, group) if group is not None else None
            c = _cfg(dims, rates, p_attn, p_aspp, seed, hook)
            grads = grad_buffer(ws, dev)
            d_cq = torch.empty_like(cq)
            ptrs, gptrs = [w.data_ptr() for w in ws], [g.data_ptr() for g in grads]
            heads = _head_struct(ptrs[nl * _PER_LAYER:], [(m.data_ptr(), v.data_ptr()) for m, v in ctx.running])
            hgrads = _lib.fill(_lib.AxvsCCHeadGrads, gptrs[nl * _PER_LAYER:])
            with _lib.train_amp(ctx.amp):
                rc = _lib.lib().axvs_cc_module_train_bwd(gl.data_ptr(), gm.data_ptr(), cq.data_ptr(), pf.data_ptr(), _layers(ptrs, nl),
                                                         C.byref(heads), _layers(gptrs, nl), C.byref(hgrads), d_cq.data_ptr(), C.byref(c),
                                                         saved_ptr, nsaved, scratch.data_ptr(), nscr, _stream(dev))
            if hook is not None and hook.error is not None:
                raise hook.error
            _lib.check(rc, "axvs_cc_module_train_bwd")
        d_cq, *grads = cast([d_cq, *grads], ctx.in_dtypes)
        return (d_cq, None, None, None, *grads)


def cc_module_train(mod, clip_query: Tensor, panoptic_features: Tensor):
    """Differentiable forward of a CrossClipTrackingModule in train() mode -> (class logits [nl,1,Q,K1], mask logits [nl,B,Q,Tc*V,H,W]);
    updates the running statistics of the module's four BatchNorm sites like the reference's forward does (once per layer)."""
    B, Q, Tc, Cq = clip_query.shape
    V = mod.num_clip_frames
    if Cq != 256 or panoptic_features.dim() != 5 or panoptic_features.shape[1] != 128:
        raise RuntimeError("clip_query must be [B,Q,T,256] and panoptic_features [B,128,T*V,H,W]")
    Bp, _, TV, H, W = panoptic_features.shape
    if Bp != B or TV != Tc * V:
        raise RuntimeError(f"panoptic_features {tuple(panoptic_features.shape)} does not match clip_query {tuple(clip_query.shape)} / V={V}")
    if panoptic_features.requires_grad:
        raise NotImplementedError("axial_vs_amd: no gradient for panoptic_features (the frozen segmenter's output, maxtron_cc_model.py:104-108); "
                                  "detach() it")
    for lay in mod.transformer_trajectory_self_attention_layers:
        if lay.normalize_before or lay.dropout.p != 0.0:
            raise NotImplementedError("axial_vs_amd: the cross-clip layer is post-norm with dropout 0 (CC:249-255)")
    bns = cc_bn_modules(mod)
    K1 = mod._predictor._transformer_class_head.conv.weight.shape[0]
    nl = mod.num_layers
    p_attn, p_aspp = float(mod.attn_drop), float(mod.aspp_drop)
    cfg = ((int(B), int(Q), int(Tc), int(V), int(H), int(W), int(K1), int(nl)), tuple(int(r) for r in mod.atrous_rates), p_attn, p_aspp,
           draw_seed(mod, p_attn, p_aspp))
    running = [(bn.running_mean, bn.running_var) for bn in bns]
    logits, masks, stats = apply(mod, _CCModuleTrain, clip_query, panoptic_features, cfg, running, *module_parameters(mod))
    # running statistics: one momentum step per layer call, in layer order (nn.BatchNorm semantics, momentum 0.01), folded into
    # one update per buffer: r <- (1-m)^nl r + sum_l m (1-m)^(nl-1-l) stat_l
    with torch.no_grad():
        off = 0
        for bn in bns:
            Cn = bn.num_features
            st = stats[off:off + nl * 2 * Cn].view(nl, 2, Cn)
            off += nl * 2 * Cn
            if not bn.track_running_stats or bn.running_mean is None:
                continue
            if bn.momentum is None:          # cumulative moving average: the factor depends on the counter, step by step
                for l in range(nl):
                    bn.num_batches_tracked += 1
                    m = 1.0 / float(bn.num_batches_tracked)
                    bn.running_mean.mul_(1 - m).add_(st[l, 0].to(bn.running_mean.dtype), alpha=m)
                    bn.running_var.mul_(1 - m).add_(st[l, 1].to(bn.running_var.dtype), alpha=m)
                continue
            m = float(bn.momentum)
            coef = torch.tensor([m * (1 - m) ** (nl - 1 - l) for l in range(nl)], dtype=torch.float32, device=st.device)
            upd = torch.einsum("l,lsc->sc", coef, st)
            bn.running_mean.mul_((1 - m) ** nl).add_(upd[0].to(bn.running_mean.dtype))
            bn.running_var.mul_((1 - m) ** nl).add_(upd[1].to(bn.running_var.dtype))
            bn.num_batches_tracked += nl
    return logits, masks


# ---- the layer chain alone: the first half of the Tube-Link head's train() mode (its prediction heads follow: tl_heads_train below) ------
class _CCLayersTrain(torch.autograd.Function):
    @staticmethod
    def forward(ctx, clip_query, cfg, *params):
        from .modules import _stream
        dims, rates, p_attn, p_aspp, seed = cfg
        require_gpu(clip_query)
        B, Q, Tc, nl = dims
        cq = f32c(clip_query)
        ws = [f32c(w) for w in params]
        dev = cq.device
        full = (B, Q, Tc, 1, 1, 1, 1, nl)
        with torch.cuda.device(dev):
            c = _cfg(full, rates, p_attn, p_aspp, seed, None)
            c.chain_only = 1
            nsaved = nbytes("axvs_cc_module_train_saved_bytes", C.byref(c))
            nscr = nbytes("axvs_cc_module_train_scratch_bytes", C.byref(c), 0)
            saved, _, scratch = place(dev, nsaved, nscr, shared=False)
            out = torch.empty(nl, B, Q, Tc, 256, dtype=torch.float32, device=dev)
            _lib.check(_lib.lib().axvs_cc_layers_train_fwd(cq.data_ptr(), out.data_ptr(), _layers([w.data_ptr() for w in ws], nl), C.byref(c),
                                                           saved.data_ptr(), nsaved, scratch.data_ptr(), nscr, _stream(dev)),
                       "axvs_cc_layers_train_fwd")
        ctx.save_for_backward(cq, *ws)
        ctx.amp = _lib.current_amp()
        ctx.cfg = (full, rates, p_attn, p_aspp, seed)
        ctx.saved_buf = saved
        ctx.in_dtypes = [t.dtype for t in (clip_query, *params)]
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_out):
        from .modules import _stream
        cq, *ws = ctx.saved_tensors
        full, rates, p_attn, p_aspp, seed = ctx.cfg
        nl = full[-1]
        dev = cq.device
        with torch.cuda.device(dev):
            g = f32c(d_out)
            c = _cfg(full, rates, p_attn, p_aspp, seed, None)
            c.chain_only = 1
            nsaved = nbytes("axvs_cc_module_train_saved_bytes", C.byref(c))
            nscr = nbytes("axvs_cc_module_train_scratch_bytes", C.byref(c), 1)
            _, saved_ptr, scratch = place(dev, nsaved, nscr, shared=False, saved=ctx.saved_buf)
            grads = grad_buffer(ws, dev)
            d_cq = torch.empty_like(cq)
            with _lib.train_amp(ctx.amp):
                _lib.check(_lib.lib().axvs_cc_layers_train_bwd(g.data_ptr(), cq.data_ptr(), _layers([w.data_ptr() for w in ws], nl),
                                                               _layers([t.data_ptr() for t in grads], nl), d_cq.data_ptr(), C.byref(c),
                                                               saved_ptr, nsaved, scratch.data_ptr(), nscr, _stream(dev)),
                           "axvs_cc_layers_train_bwd")
        d_cq, *grads = cast([d_cq, *grads], ctx.in_dtypes)
        return (d_cq, None, *grads)


def cc_layers_train(mod, clip_query: Tensor, num_layers: int, rates, p_attn: float, p_aspp: float) -> Tensor:
    """Differentiable layer chain of a cross-clip module (clip_query [B,Q,Tc,256]) -> the clip queries after every layer [nl,B,Q,Tc,256]."""
    B, Q, Tc, Cq = clip_query.shape
    if Cq != 256:
        raise RuntimeError("clip_query must be [B,Q,Tc,256]")
    cfg = ((int(B), int(Q), int(Tc), int(num_layers)), tuple(int(r) for r in rates), float(p_attn), float(p_aspp),
           draw_seed(mod, p_attn, p_aspp))
    return apply(mod, _CCLayersTrain, clip_query, cfg, *chain_parameters(mod, num_layers))


# ---- the Tube-Link head's prediction heads, all layers at once (axvs_tl_heads_train_*) ------------------------------------------------
def tl_heads_cfg(nl: int, B: int, Q: int, Tc: int, fpc: int, h: int, w: int, K1: int, Cm: int) -> _lib.AxvsTLHeadTrainCfg:
    return _lib.AxvsTLHeadTrainCfg(int(B), int(Q), int(Tc), int(fpc), int(h), int(w), int(K1), int(Cm), int(nl))


def tl_heads_supported(cfg: _lib.AxvsTLHeadTrainCfg) -> bool:
    """True when the library's bounds take this configuration (else axvs_last_error() names the bound)."""
    return _lib.lib().axvs_tl_heads_train_saved_bytes(C.byref(cfg)) > 0


class _TLHeadsTrain(torch.autograd.Function):
    @staticmethod
    def forward(ctx, queries, mask_features, dims, *params):
        from .modules import _stream
        require_gpu(queries)
        nl, B, Q, Tc, fpc, h, w, K1, Cm = dims
        qs, mf = f32c(queries), f32c(mask_features)
        ws = [f32c(p) for p in params]
        dev = qs.device
        with torch.cuda.device(dev):
            c = tl_heads_cfg(*dims)
            nsaved = nbytes("axvs_tl_heads_train_saved_bytes", C.byref(c))
            nscr = nbytes("axvs_tl_heads_train_scratch_bytes", C.byref(c), 0)
            saved, _, scratch = place(dev, nsaved, nscr, shared=False)
            cls = torch.empty(nl, B, Q, K1, dtype=torch.float32, device=dev)
            masks = torch.empty(nl, B, Tc * fpc, Q, h, w, dtype=torch.float32, device=dev)
            hp = _lib.fill(_lib.AxvsTLHeadParams, [t.data_ptr() for t in ws])
            _lib.check(_lib.lib().axvs_tl_heads_train_fwd(qs.data_ptr(), mf.data_ptr(), cls.data_ptr(), masks.data_ptr(), C.byref(hp), C.byref(c),
                                                          saved.data_ptr(), nsaved, scratch.data_ptr(), nscr, _stream(dev)),
                       "axvs_tl_heads_train_fwd")
        ctx.save_for_backward(qs, mf, *ws)
        ctx.amp = _lib.current_amp()
        ctx.dims = dims
        ctx.saved_buf = saved
        ctx.in_dtypes = [t.dtype for t in (queries, mask_features, *params)]
        return cls, masks

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_cls, d_masks):
        from .modules import _stream
        qs, mf, *ws = ctx.saved_tensors
        nl, B, Q, Tc, fpc, h, w, K1, Cm = ctx.dims
        dev = qs.device
        with torch.cuda.device(dev):
            gc = f32c(d_cls) if d_cls is not None else torch.zeros(nl, B, Q, K1, dtype=torch.float32, device=dev)
            gm = f32c(d_masks) if d_masks is not None else torch.zeros(nl, B, Tc * fpc, Q, h, w, dtype=torch.float32, device=dev)
            c = tl_heads_cfg(*ctx.dims)
            nsaved = nbytes("axvs_tl_heads_train_saved_bytes", C.byref(c))
            nscr = nbytes("axvs_tl_heads_train_scratch_bytes", C.byref(c), 1)
            _, saved_ptr, scratch = place(dev, nsaved, nscr, shared=False, saved=ctx.saved_buf)
            grads = grad_buffer(ws, dev)
            d_q = torch.empty_like(qs)
            d_mf = torch.empty_like(mf) if ctx.needs_input_grad[1] else None
            hp = _lib.fill(_lib.AxvsTLHeadParams, [p.data_ptr() for p in ws])
            hg = _lib.fill(_lib.AxvsTLHeadGrads, [g.data_ptr() for g in grads])
            with _lib.train_amp(ctx.amp):
                _lib.check(_lib.lib().axvs_tl_heads_train_bwd(gc.data_ptr(), gm.data_ptr(), qs.data_ptr(), mf.data_ptr(), C.byref(hp), C.byref(hg),
                                                              d_q.data_ptr(), d_mf.data_ptr() if d_mf is not None else None, C.byref(c),
                                                              saved_ptr, nsaved, scratch.data_ptr(), nscr, _stream(dev)),
                           "axvs_tl_heads_train_bwd")
        d_q, d_mf, *grads = cast([d_q, d_mf, *grads], ctx.in_dtypes)
        return (d_q, d_mf, None, *grads)


def tl_heads_train(mod, queries: Tensor, mask_features: Tensor, cfg: _lib.AxvsTLHeadTrainCfg):
    """Differentiable prediction heads of a TubeLinkCrossClipHead for every layer: queries [nl,B,Q,Tc,256] (cc_layers_train's output),
    mask_features [B,Tc*fpc,Cm,h,w] -> (class logits [nl,B,Q,K1], mask logits [nl,B,Tc*fpc,Q,h,w]).  `cfg` from tl_heads_cfg, accepted
    by tl_heads_supported."""
    dims = (cfg.num_layers, cfg.B, cfg.Q, cfg.Tc, cfg.frames_per_clip, cfg.h, cfg.w, cfg.K1, cfg.Cm)
    return apply(mod, _TLHeadsTrain, queries, mask_features, dims, *tl_heads_parameters(mod))
