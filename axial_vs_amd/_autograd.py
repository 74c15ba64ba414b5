"""Host plumbing of the training tier's autograd Functions (training.py, cc_training.py, glue_training.py): how a call gets its buffers,
its precision and its dropout seed.  Each Function keeps its own forward / backward with its library call written out; nothing here
computes anything.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import torch
from torch import Tensor

from . import _lib


def f32c(t: Optional[Tensor]) -> Optional[Tensor]:
    """`t` detached, fp32 and contiguous (None stays None)."""
    if t is None:
        return None
    t = t.detach()
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def require_gpu(t: Tensor) -> None:
    if not t.is_cuda:
        raise RuntimeError("axial_vs_amd: the training tier needs GPU tensors; there is no CPU fallback")


def nbytes(query: str, *args) -> int:
    """The library's size query `query`(*args).  0 means the library refused the configuration: raised with its reason."""
    L = _lib.lib()
    n = getattr(L, query)(*args)
    if n == 0:
        raise RuntimeError(query + ": " + L.axvs_last_error().decode())
    return n


def place(dev, nsaved: int, nscr: int, recompute: bool = False, shared: bool = True, saved: Optional[Tensor] = None):
    """Where a call's saved activations and scratch go -> (saved tensor or None, saved pointer, scratch tensor).

    Scratch comes from the shared workspace (`shared`) or from a private tensor.  Under `recompute` (shared scratch only) the saved
    activations are scratch too: they sit in the shared workspace after the scratch part, and no saved tensor is returned.  Otherwise
    they are `saved` (the backward: the forward's tensor) or a new private tensor (the forward), which the Function keeps on ctx."""
    from .modules import _workspace
    if recompute:
        buf = _workspace(dev, nscr + nsaved)
        return None, buf.data_ptr() + nscr, buf
    if saved is None:
        saved = torch.empty(nsaved, dtype=torch.uint8, device=dev)
    scratch = _workspace(dev, nscr) if shared else torch.empty(nscr, dtype=torch.uint8, device=dev)
    return saved, saved.data_ptr(), scratch


def grad_buffer(params: Sequence[Tensor], dev) -> List[Tensor]:
    """Gradient buffers for `params`: one flat fp32 tensor, one view per parameter shaped like it."""
    flat = torch.empty(sum(p.numel() for p in params), dtype=torch.float32, device=dev)
    return [g.view(p.shape) for g, p in zip(flat.split([p.numel() for p in params]), params)]


def cast(grads: Sequence[Optional[Tensor]], dtypes) -> List[Optional[Tensor]]:
    """Gradients back in their inputs' dtypes (None stays None)."""
    return [None if g is None else g.to(dt) for g, dt in zip(grads, dtypes)]


def apply(owner, fn, *args):
    """`fn.apply(*args)` with autocast switched off for the call.  Under autocast the library's GEMMs take the autocast dtype
    (library option train_amp, read from `owner` before autocast is switched off); the Function keeps it for its backward."""
    if torch.is_autocast_enabled():
        amp = _lib.autocast_mode(owner)
        with torch.autocast(device_type="cuda", enabled=False), _lib.train_amp(amp):
            return fn.apply(*args)
    return fn.apply(*args)


def draw_seed(owner, *probs: float) -> int:
    """The dropout seed of a call: `owner.dropout_seed`, else one draw from torch's CPU generator when a dropout probability is above 0
    (0 otherwise, and the generator is left alone)."""
    s = getattr(owner, "dropout_seed", None)
    if s is None:
        s = int(torch.randint(0, 2 ** 31 - 1, (1,)).item()) if any(p > 0 for p in probs) else 0
    return int(s)
