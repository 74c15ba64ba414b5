"""Video instance post-processing on the device for Tube-Link VIS: both resizes, threshold, mask scores, boxes, per-frame top-k, masks.

Reference (MaXTron_Tube-Link): `Mask2FormerVideoCCHeadTube.simple_test` (models/video/tube_link_vis/mask2former_video_cc_head.py:
1003-1036) resizes the [T, Q, h, w] mask logits of the whole video to `batch_input_shape`; `TubeLinkVideoVIS.simple_test`
(mask2former_vis_video.py:160-211) drops the padded frames and calls, frame by frame, `MaskFormerFusionHead.simple_test` ->
`instance_postprocess` (mmdet/models/seg_heads/panoptic_fusion_heads/maskformer_fusion_head.py:405-462, 509-568): crop to `img_shape`,
`topk` over the Q x C class scores, a second `F.interpolate` to `ori_shape`, `> 0`, the mean sigmoid inside each mask, `mask2bbox`
(mmdet/core/mask/utils.py:68-89: a Python loop with two host synchronisations per mask); the caller then sorts by detection score and
keeps 30.  Here all of it runs in libaxvs.so in four kernels and one memset (axial_vs_amd/csrc/axvs_vis.h); no resized [T, Q, H, W] tensor exists.

Deviations from the reference, both where it leaves the result open:
  * `topk(sorted=False)` fixes no candidate order; here candidates come in DESCENDING class score, equal scores to the lower flat
    index `query * C + label`;
  * equal detection scores (in practice the empty masks: all 0) go to the lower candidate position.
An instance id is 1 + the position in the candidate list, the same in every frame, so the ids are a permutation of the reference's
within a video -- immaterial to a VIS evaluation, which only links equal ids across frames.

Run-length encoding (`encode_mask_results`, pycocotools) stays with the caller: masks come back as numpy bool arrays, as the reference
holds them just before it encodes.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib
from .matching import _mask_dtype
from .modules import _guarded, _stream, _workspace_for


def _al(n: int) -> int:
    return (n + 15) // 16 * 16


def unpack_bits(words, W: int):
    """`mask_format="bits"` words int64 [..., ceil(W/64)] (torch tensor or numpy array) -> bool [..., W]: bit i of word j is pixel
    64 j + i of the row."""
    if isinstance(words, Tensor):
        sh = torch.arange(64, device=words.device, dtype=torch.int64)
        return (((words.unsqueeze(-1) >> sh) & 1) != 0).flatten(-2)[..., :W]
    b = np.unpackbits(np.ascontiguousarray(words).view(np.uint8), axis=-1, bitorder="little")      # little-endian words: byte k = bits 8k..8k+7
    return b[..., :W].astype(bool)


def _layout(F: int, K: int, Ko: int):
    """(int32 fields, fp32 fields) as (name, shape) in the order include/axvs.h states for table_ints / table_floats"""
    ints = [("counts", (2,)),                                                        # candidates kept (things), queries they refer to
            ("cand_query", (K,)), ("cand_label", (K,)),                              # the candidate list, tail -1
            ("area", (F, K)),                                                        # per frame and candidate
            ("count", (F,)), ("track_id", (F, Ko)), ("label", (F, Ko)), ("query", (F, Ko))]      # per frame: the selection
    floats = [("cand_cls_score", (K,)), ("mask_score", (F, K)), ("det_score", (F, K)), ("cand_bbox", (F, K, 4)), ("bbox", (F, Ko, 4)), ("score", (F, Ko))]
    return ints, floats


def _offsets(F: int, K: int, Ko: int, H: int, W: int, bits: bool):
    """byte offsets in the one output buffer: (int table, fp32 table, masks, end), and the two tables' element counts"""
    ni, nf = (sum(int(np.prod(shape)) for _, shape in fields) for fields in _layout(F, K, Ko))
    o1 = _al(4 * ni)
    o2 = o1 + _al(4 * nf)
    return (0, o1, o2, o2 + (F * Ko * H * ((W + 63) // 64) * 8 if bits else F * Ko * H * W)), ni, nf


def _views(buf: Tensor, F: int, K: int, Ko: int, H: int, W: int, bits: bool):
    """the one output buffer (uint8) as (masks, int table, float table, dict of named views)"""
    (o0, o1, o2, end), ni, nf = _offsets(F, K, Ko, H, W, bits)
    ti, tf = buf[o0:o0 + 4 * ni].view(torch.int32), buf[o1:o1 + 4 * nf].view(torch.float32)
    masks = buf[o2:end].view(torch.int64).view(F, Ko, H, (W + 63) // 64) if bits else buf[o2:end].view(F, Ko, H, W)
    tables = {}
    for t, fields in zip((ti, tf), _layout(F, K, Ko)):
        o = 0
        for name, shape in fields:
            n = int(np.prod(shape))
            tables[name] = t[o:o + n].view(*shape)
            o += n
    return masks, ti, tf, tables


def _launch(mask_cls: Tensor, mask_pred: Tensor, num_frames, batch_input_shape, img_shape, ori_shape, num_things_classes, max_per_image,
            keep_per_frame, mask_format):
    if not mask_cls.is_cuda or not mask_pred.is_cuda:
        raise RuntimeError(f"axial_vs_amd: mask_cls / mask_pred must be GPU tensors (got {mask_cls.device}, {mask_pred.device}); there is no CPU fallback")
    if mask_pred.dim() != 4 or mask_cls.dim() != 2 or mask_cls.shape[0] != mask_pred.shape[1]:
        raise RuntimeError(f"mask_pred {tuple(mask_pred.shape)} must be [T, Q, h, w] and mask_cls {tuple(mask_cls.shape)} [Q, C + 1]")
    if mask_format not in ("uint8", "bits"):
        raise RuntimeError(f"mask_format {mask_format!r} must be 'uint8' or 'bits'")
    if mask_pred.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        mask_pred = mask_pred.float()
    mask_pred, mask_cls = mask_pred.contiguous(), mask_cls.float().contiguous()
    dev = mask_pred.device
    T, Q, h, w = mask_pred.shape
    F = T if num_frames is None else int(num_frames)
    K, Ko, bits = int(max_per_image), int(keep_per_frame), mask_format == "bits"
    H, W = int(ori_shape[0]), int(ori_shape[1])
    cfg = _lib.AxvsVisCfg(Q=Q, K1=mask_cls.shape[1], T=T, num_frames=F, h=h, w=w, image_h=int(batch_input_shape[0]), image_w=int(batch_input_shape[1]),
                          crop_h=int(img_shape[0]), crop_w=int(img_shape[1]), H=H, W=W, num_things=int(num_things_classes), k_cand=K, k_out=Ko,
                          mask_bits=int(bits))
    L = _lib.lib()
    st = _stream(dev)
    ws = _workspace_for("axvs_video_instance_workspace_bytes", dev, st, C.byref(cfg))
    buf = torch.empty(_offsets(F, K, Ko, H, W, bits)[0][3], dtype=torch.uint8, device=dev)      # tables and masks: one buffer, one copy to the host
    masks, ti, tf, tables = _views(buf, F, K, Ko, H, W, bits)
    _lib.check(L.axvs_video_instance_fwd(C.byref(cfg), mask_cls.data_ptr(), mask_pred.data_ptr(), _mask_dtype(mask_pred), masks.data_ptr(),
                                         ti.data_ptr(), tf.data_ptr(), ws.data_ptr(), ws.numel(), st), "axvs_video_instance_fwd")
    return buf, masks, tables, (F, K, Ko, H, W, bits)


@_guarded
@torch.no_grad()
def video_instance_inference(mask_cls: Tensor, mask_pred: Tensor, *, batch_input_shape: Tuple[int, int], img_shape: Tuple[int, int],
                             ori_shape: Tuple[int, int], num_things_classes: int, num_frames: int = None, max_per_image: int = 100,
                             keep_per_frame: int = 30, mask_format: str = "uint8", return_tables: bool = False):
    """The instance branch of `TubeLinkVideoVIS.simple_test` for ONE video, from the head's last-layer outputs before any resize:
    mask_cls [Q, C + 1], mask_pred [T, Q, h, w] (fp32, fp16 or bf16; arithmetic in fp32), GPU tensors -- there is no CPU fallback.
    Frames `num_frames..T-1` are padding and are dropped (`mask_pred_results[:, :-pad_size]`).  Bilinear resize h x w ->
    `batch_input_shape`, crop to `img_shape`, bilinear resize -> `ori_shape` (both align_corners=False); candidates = the
    `max_per_image` largest of the Q x C softmax scores with label < `num_things_classes`, once per video; per frame the
    `keep_per_frame` candidates with the largest detection score (class score x mean sigmoid inside the mask).

    Returns `(masks, tables)`.  `masks`: uint8 [num_frames, keep_per_frame, H, W], or with `mask_format="bits"` int64
    [num_frames, keep_per_frame, H, ceil(W/64)] (bit i of word j = pixel 64 j + i; `unpack_bits` undoes it).  `tables`: per frame
    `count`, and padded with -1 to keep_per_frame `track_id` (1 + candidate position: the same id in every frame), `label`, `query`,
    `bbox` fp32 [., 4] = (xmin, ymin, xmax + 1, ymax + 1) or zeros for an empty mask, `score`; the candidate list `cand_query`,
    `cand_label`, `cand_cls_score`; per frame and candidate `area` (exact, int32), `mask_score`, `det_score`, `cand_bbox`; `counts`.
    By default masks and tables are numpy arrays read back in ONE device-to-host copy (the one synchronisation of the call);
    `return_tables=True` returns device tensors and does not synchronise.

    Two deviations, where the reference leaves the result open: candidates are in descending class score with equal scores to the
    lower flat index (the reference's `topk(sorted=False)` has no fixed order), and equal detection scores go to the lower candidate
    position -- so ids are a permutation of the reference's within a video.  Q <= 512, Q*C <= 2^17,
    keep_per_frame <= max_per_image <= min(Q*C, 256).  Run-length encoding of the masks stays with the caller."""
    buf, masks, tables, dims = _launch(mask_cls, mask_pred, num_frames, batch_input_shape, img_shape, ori_shape, num_things_classes, max_per_image,
                                       keep_per_frame, mask_format)
    if return_tables:
        return masks, tables
    host = torch.empty(buf.shape, dtype=torch.uint8, pin_memory=True)       # (torch caches pinned blocks: no allocation after the first call)
    host.copy_(buf, non_blocking=True)                      # the one copy: tables and masks together, to pinned memory at link speed
    torch.cuda.current_stream(buf.device).synchronize()     # the one synchronisation
    masks, _, _, tables = _views(host, *dims)
    return masks.numpy(), {k: v.numpy() for k, v in tables.items()}


class VideoInstancePostProcessor:
    """Drop-in for the instance branch of `TubeLinkVideoVIS.simple_test` (mask2former_vis_video.py:160-201): called with the head's
    last-layer outputs `mask_cls_results [B, Q, C + 1]`, `mask_pred_results [B, T, Q, h, w]` BEFORE the head's resize, the
    `ref_img_metas` and the number of real frames; returns `results[b][frame] = {'ins_results': (bbox_results, mask_results)}` as the
    reference holds them just before `encode_mask_results`: `bbox_results` per class as `bbox2result` lays them out (rows
    `[id, x1, y1, x2, y2, score]`), `mask_results` per class a list of numpy bool [H, W] masks.  One device-to-host copy per video;
    run-length encoding stays with the caller."""

    def __init__(self, num_things_classes: int, max_per_image: int = 100, keep_per_frame: int = 30):
        self.num_things_classes, self.max_per_image, self.keep_per_frame = int(num_things_classes), int(max_per_image), int(keep_per_frame)

    @classmethod
    def from_model(cls, model) -> "VideoInstancePostProcessor":
        """from a reference detector (its `panoptic_fusion_head`) or a fusion head: `num_things_classes` and `test_cfg.max_per_image`"""
        head = getattr(model, "panoptic_fusion_head", model)
        return cls(head.num_things_classes, (head.test_cfg or {}).get("max_per_image", 100))

    def per_class(self, masks: np.ndarray, tb: Dict[str, np.ndarray], frame: int, W: int):
        n = int(tb["count"][frame])
        labels = tb["label"][frame, :n]
        if n == 0:
            bbox_results = [np.zeros((0, 5), dtype=np.float32) for _ in range(self.num_things_classes)]
        else:
            rows = np.concatenate([tb["track_id"][frame, :n, None].astype(np.float32), tb["bbox"][frame, :n], tb["score"][frame, :n, None]], axis=1)
            bbox_results = [rows[labels == i, :] for i in range(self.num_things_classes)]
        mask_results: List[List[np.ndarray]] = [[] for _ in range(self.num_things_classes)]
        full = unpack_bits(masks[frame, :n], W)
        for j, label in enumerate(labels):
            mask_results[label].append(full[j])
        return bbox_results, mask_results

    def __call__(self, mask_cls_results: Tensor, mask_pred_results: Tensor, ref_img_metas: Sequence[Sequence[dict]], num_frames: int = None):
        results = []
        for b in range(mask_cls_results.shape[0]):
            meta = ref_img_metas[b][0]
            H, W = meta["ori_shape"][:2]
            masks, tb = video_instance_inference(mask_cls_results[b], mask_pred_results[b], batch_input_shape=meta["batch_input_shape"],
                                                 img_shape=meta["img_shape"][:2], ori_shape=(H, W), num_things_classes=self.num_things_classes,
                                                 num_frames=num_frames, max_per_image=self.max_per_image, keep_per_frame=self.keep_per_frame,
                                                 mask_format="bits")
            results.append([{"ins_results": self.per_class(masks, tb, f, W)} for f in range(masks.shape[0])])
        return results
