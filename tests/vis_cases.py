"""Cases, input recipe, restatement and screens of the video instance post-processing tests (tests/test_vis_cpu.py,
tests/test_hip_vis.py, tools/gen_golden_vis.py).

`restate` re-types the op sequence of MaXTron_Tube-Link's VIS inference tail in the dtype of its inputs:
`F.interpolate` to batch_input_shape (models/video/tube_link_vis/mask2former_video_cc_head.py:1026-1034), the drop of the padded frames
and the per-frame loop (mask2former_vis_video.py:162-193), the crop to img_shape (maskformer_fusion_head.py:512-513),
`instance_postprocess` (:426-462: softmax, topk, the thing filter, `F.interpolate` to ori_shape, `> 0`, the mean sigmoid, `mask2bbox`) and
the caller's argsort and `[:30]`.  Run in float64 it is the yardstick the device is compared with; run in float32 it is the reference's
own arithmetic, whose distance from float64 sizes the screens and the score tolerance.  The two additions are the tie rules the
reference leaves open: candidates in descending class score with equal scores to the lower flat index (`topk(sorted=False)` fixes no
order), and equal detection scores to the lower candidate position (a stable argsort).

The outputs are discrete, so the cases are SCREENED and then compared exactly (`screen`).  A seed is accepted if
  * no doubly-resized float64 logit of a candidate lies within `band = 8 x max |fp32 - fp64|` of 0 (8: the project's usual margin for
    another interpolation and summation order),
  * the top K_cand + 1 class scores are pairwise at least 1e-5 apart (relative),
  * the non-zero detection scores of each frame are pairwise at least 1e-5 apart (relative),
  * the fp32 restatement reproduces the float64 masks, candidates and selection exactly.
Seeds are tried in order; the first that passes is pinned in tests/golden/g21_vis_seeds.json.  In the multi-tile cases (e, h) no seed keeps
millions of logits outside the band by chance, so `find_seed` first raises the offending low-resolution logits by 0.25 (the nudge of
panoptic_cases.find_seed) and then applies the screens unchanged.
"""
import functools
import json
import os
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

from panoptic_cases import GOLDEN

Case = namedtuple("Case", "name Q C T h w bi img ori K Ko F things empty bf16", defaults=(False,))

# (Q, C, T, h x w, batch_input, img_shape, ori_shape, K_cand, K_out); F: the real frames (num_frames); things: num_things_classes;
# empty: queries whose logits are all negative (empty masks: area 0, score 0, zero box -- the tie rule of the selection at work);
# bf16: the stored logits are bf16 values (which fp16 and fp32 hold as well) instead of fp16 values
CASES = [
    Case("a", 3, 2, 1, 4, 5, (16, 20), (14, 19), (9, 11), 4, 3, 1, 2, 2),              # second stage shrinks; W < 64
    Case("b", 16, 7, 2, 6, 10, (24, 40), (22, 37), (45, 75), 20, 5, 2, 7, 0),          # non-integer enlargement; W = 75: a ragged second word
    Case("c", 100, 40, 3, 8, 8, (32, 32), (32, 32), (32, 32), 100, 30, 3, 40, 60),     # the shipped Q, C, K; no crop; identity second stage
    Case("d", 20, 10, 1, 7, 9, (28, 36), (25, 33), (50, 70), 100, 30, 1, 10, 6),       # half the candidates share queries; six queries empty
    Case("e", 32, 40, 2, 24, 40, (96, 160), (90, 160), (180, 320), 100, 30, 2, 40, 8), # many tiles per frame: atomics across workgroups
    Case("f", 40, 5, 1, 40, 48, (40, 48), (40, 48), (20, 24), 50, 10, 1, 5, 0),        # shrinking resize: the global-tap path of both passes
    Case("g", 16, 7, 5, 6, 10, (24, 40), (22, 37), (45, 75), 20, 5, 3, 7, 0),          # as b with num_frames 3 < T 5: dropped frames are inert
    Case("c25", 100, 40, 3, 8, 8, (32, 32), (32, 32), (32, 32), 100, 30, 3, 25, 60),   # c with 25 thing classes: the filter and the compaction
    Case("b16", 16, 7, 2, 6, 10, (24, 40), (22, 37), (45, 75), 20, 5, 2, 7, 0, True),  # b's geometry on bf16 values: the bf16 loader, screened
    # e's geometry over 20 frames: 225 tiles x 20 frames > 2048 workgroups, so a workgroup runs over three tiles -- the staging tile
    # reused behind barriers, the LDS accumulators kept over the run, the emit tail's loop over tiles (every shipped size runs so)
    Case("h", 8, 5, 20, 24, 40, (96, 160), (90, 160), (180, 320), 8, 4, 20, 5, 2),
    Case("k", 128, 40, 1, 4, 5, (16, 20), (14, 19), (9, 11), 20, 5, 1, 40, 3),         # Q*C = 5120 > 4096: the candidate keys in global memory
]
# Of case d's 100 candidates at most 6 x 10 refer to its six empty queries, so at least 40 have area and its selection holds no zero
# score; a zero score is selected while another is not -- the tie rule decides -- in cases a and c25 (tests/test_vis_cpu.py asserts it
# on the pinned seeds).
BY_NAME = {c.name: c for c in CASES}
FIXTURE_CASES = [BY_NAME[n] for n in "abcd"]      # stored with the reference's own results (tests/golden/g21_vis_*.npz)
MULTI_TILE = BY_NAME["e"]
NUDGED = (BY_NAME["e"], BY_NAME["h"])       # millions of resized logits: no seed keeps them all outside the band by chance
SEED0 = 21000
MAX_SEEDS = 64
MAX_ROUNDS = 30
PINNED = os.path.join(GOLDEN, "g21_vis_seeds.json")


def case_name(c):
    return "g21_vis_" + c.name


def _stored(c, mp):
    """the logits as the case stores them: fp16 values, or bf16 values"""
    return mp.bfloat16().float() if c.bf16 else mp.half().float()


def make_inputs(c, seed):
    """(mask_cls [Q, C+1], mask_pred [T, Q, h, w]), fp32 holding fp16 values.  Logits randn * 4; the first `empty` odd queries are all
    negative; every fifth query is a copy of its predecessor plus 0.05 randn; class logits randn * 2 (an empty query's class logits are
    raised by 3 so that empty masks reach the candidate list and, in cases a and c25, the selection)."""
    g = torch.Generator().manual_seed(seed)
    mp = torch.randn(c.T, c.Q, c.h, c.w, generator=g) * 4.0
    for q in range(4, c.Q, 5):
        mp[:, q] = mp[:, q - 1] + 0.05 * torch.randn(c.T, c.h, c.w, generator=g)
    cls = torch.randn(c.Q, c.C + 1, generator=g) * 2.0
    for q in list(range(1, c.Q, 2))[:c.empty] + list(range(0, c.Q, 2))[:max(0, c.empty - c.Q // 2)]:
        mp[:, q] = -(mp[:, q].abs() + 0.5)
        cls[q, :c.C] += 3.0
    return cls.half().float(), _stored(c, mp)


def mask2bbox(masks):
    """mmdet/core/mask/utils.py:68-89 without its Python loop: first and last set column / row, zeros for an empty mask"""
    n, H, W = masks.shape
    x_any, y_any = masks.any(dim=1), masks.any(dim=2)
    out = torch.zeros(n, 4, dtype=torch.float32)
    some = x_any.any(dim=1)
    out[:, 0] = x_any.int().argmax(dim=1)
    out[:, 1] = y_any.int().argmax(dim=1)
    out[:, 2] = W - x_any.flip(1).int().argmax(dim=1)
    out[:, 3] = H - y_any.flip(1).int().argmax(dim=1)
    out[~some] = 0
    return out


def candidates(c, cls):
    """instance_postprocess:429-444 with the candidate order fixed: (flat indices, scores, labels, queries) after the thing filter, and
    the K_cand + 1 largest scores before it"""
    scores = F.softmax(cls, dim=-1)[:, :-1].flatten(0, 1)
    top, idx = torch.sort(scores, descending=True, stable=True)          # topk(K) with equal scores to the lower flat index
    lead = top[:c.K + 1]
    top, idx = top[:c.K], idx[:c.K]
    labels, query = idx % c.C, idx // c.C
    keep = labels < c.things
    return idx[keep], top[keep], labels[keep], query[keep], lead


def resized(c, mp, query, t):
    """frame t of the candidates' logits after both resizes, [n, H, W]; the first resize runs on the whole frame as the head does"""
    up = F.interpolate(mp[t:t + 1], size=c.bi, mode="bilinear", align_corners=False)[0]
    up = up[query][:, :c.img[0], :c.img[1]]
    return F.interpolate(up.unsqueeze(0), size=c.ori, mode="bilinear", align_corners=False).squeeze(0)


def restate(c, inputs, dtype=torch.float64, keep_logits=False):
    """The reference's op sequence in `dtype`.  Returns a namespace: the candidate list (`query`, `label`, `cls_score`) and per real
    frame `area` int64 [n], `mask_score`, `det_score` [n], `bbox` fp32 [n, 4], `binary` bool [n, H, W], `sel` (candidate positions of
    the K_out rows in order; instance id = position + 1)."""
    cls, mp = (x.to(dtype) for x in inputs)
    idx, sc, labels, query, lead = candidates(c, cls)
    out = SimpleNamespace(flat=idx, query=query, label=labels, cls_score=sc, lead=lead, frames=[])
    for t in range(c.F):                                                  # mask_pred_results[:, :-pad_size], then frame by frame
        m = resized(c, mp, query, t)
        binary = (m > 0).to(dtype)
        ms = (m.sigmoid() * binary).flatten(1).sum(1) / (binary.flatten(1).sum(1) + 1e-6)
        det = sc * ms
        b = binary.bool()
        sel = torch.argsort(det, descending=True, stable=True)[:c.Ko]     # equal scores to the lower candidate position
        out.frames.append(SimpleNamespace(area=b.flatten(1).sum(1), mask_score=ms, det_score=det, bbox=mask2bbox(b), binary=b, sel=sel,
                                          logits=m if keep_logits else None))
    return out


def _rel_gap(v):
    v = v.double().sort().values
    return float(((v[1:] - v[:-1]) / v[1:]).min()) if len(v) > 1 else float("inf")


def screen(c, inputs):
    """(ok, why, stats): the screens of the module docstring; `stats` keeps the fp32 errors (resized logits, mask score, detection
    score, class score) and counts what the float64 run shows"""
    r64, r32 = restate(c, inputs, torch.float64, keep_logits=True), restate(c, inputs, torch.float32, keep_logits=True)
    st = dict(err=0.0, ms_err=0.0, det_err=0.0, cls_err=0.0, shared=0, empty_cands=0, zero_selected=0, ncand=len(r64.query))
    if _rel_gap(r64.lead) < 1e-5:
        return False, "two of the top K_cand + 1 class scores closer than 1e-5", st
    if not (torch.equal(r32.flat, r64.flat)):
        return False, "the fp32 candidates differ from float64", st
    st["cls_err"] = float((r32.cls_score.double() - r64.cls_score).abs().max()) if len(r64.query) else 0.0
    st["shared"] = len(r64.query) - len(set(r64.query.tolist()))
    for t, (f64, f32) in enumerate(zip(r64.frames, r32.frames)):
        err = float((f32.logits.double() - f64.logits).abs().max()) if f64.logits.numel() else 0.0
        st["err"] = max(st["err"], err)
        if f64.logits.numel() and bool((f64.logits.abs() <= 8.0 * err).any()):
            return False, f"frame {t}: a resized logit within {8.0 * err:.1e} of 0", st
        nz = f64.det_score[f64.det_score != 0]
        if _rel_gap(nz) < 1e-5:
            return False, f"frame {t}: two detection scores closer than 1e-5", st
        if not (torch.equal(f32.binary, f64.binary) and torch.equal(f32.sel, f64.sel)):
            return False, f"frame {t}: the fp32 restatement and float64 differ", st
        st["ms_err"] = max(st["ms_err"], float((f32.mask_score.double() - f64.mask_score).abs().max()))
        st["det_err"] = max(st["det_err"], float((f32.det_score.double() - f64.det_score).abs().max()))
        st["empty_cands"] += int((f64.area == 0).sum())
        st["zero_selected"] += int((f64.det_score[f64.sel] == 0).sum())
    return True, "", st


def nudged(inputs, nudges):
    """`inputs` with 0.25 added to the low-resolution logits [t, q, r, c] listed in `nudges` (still fp16 values; only fp16 cases are nudged)"""
    mp = inputs[1].clone()
    for t, q, r, col in nudges:
        mp[t, q, r, col] += 0.25
    return inputs[0], mp.half().float()


def _near(c, inputs):
    """(frame, query, low-resolution row, column) nearest to every candidate pixel whose float64 logit lies within 10x the fp32 error
    of 0 (a little wider than the screen's 8x, so that a repaired input stays clear of it)"""
    r64, r32 = restate(c, inputs, torch.float64, keep_logits=True), restate(c, inputs, torch.float32, keep_logits=True)
    out = set()
    for t, (f64, f32) in enumerate(zip(r64.frames, r32.frames)):
        err = float((f32.logits.double() - f64.logits).abs().max())
        for n, y, x in (f64.logits.abs() <= 10.0 * err).nonzero().tolist():
            yy, xx = (y + 0.5) * c.img[0] / c.ori[0] - 0.5, (x + 0.5) * c.img[1] / c.ori[1] - 0.5
            r, q = (yy + 0.5) * c.h / c.bi[0] - 0.5, (xx + 0.5) * c.w / c.bi[1] - 0.5
            out.add((t, int(r64.query[n]), min(max(int(round(r)), 0), c.h - 1), min(max(int(round(q)), 0), c.w - 1)))
    return sorted(out)


def find_seed(c, start=0):
    """(seed offset, nudges, stats) of the first seed in start .. MAX_SEEDS - 1 that passes `screen`; only the cases of NUDGED are
    repaired first (see the module docstring) -- the others must pass as drawn."""
    why = []
    for s in range(start, MAX_SEEDS):
        base, nudges = make_inputs(c, SEED0 + s), []
        if c in NUDGED:
            for _ in range(MAX_ROUNDS):
                more = _near(c, nudged(base, nudges))
                if not more:
                    break
                nudges += more
        ok, w, st = screen(c, nudged(base, nudges))
        if ok:
            return s, nudges, st
        why.append(w)
    raise AssertionError(f"{case_name(c)}: no seed in {start}..{MAX_SEEDS - 1} passes the screens: {why[-5:]}")


@functools.lru_cache(maxsize=None)
def pinned(c):
    """(seed offset, nudges) of the case, as tools/gen_golden_vis.py found and stored them"""
    with open(PINNED) as f:
        p = json.load(f)[case_name(c)]
    return p["seed"], [tuple(x) for x in p["nudges"]]


@functools.lru_cache(maxsize=None)
def inputs_of(c):
    """the case's inputs at its pinned seed: (mask_cls [Q, C+1], mask_pred [T, Q, h, w]).  Do not modify."""
    seed, nudges = pinned(c)
    return nudged(make_inputs(c, SEED0 + seed), nudges)


@functools.lru_cache(maxsize=None)
def restated(c, dtype=torch.float64):
    """restatement of the case at its pinned seed, computed once and shared.  Do not modify."""
    return restate(c, inputs_of(c), dtype)


def load_fixture(c):
    """the reference's own results: (meta, inputs, per real frame a namespace of `rows` float64 [n, 8] = (reference id, query, label,
    x1, y1, x2, y2, score) in the reference's score order and `masks` bool [n, H, W])"""
    z = np.load(os.path.join(GOLDEN, case_name(c) + ".npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    inputs = tuple(torch.from_numpy(z[k].astype(np.float32)) for k in ("mask_cls", "mask_pred"))
    H, W = c.ori
    frames = []
    for t in range(c.F):
        rows = z[f"f{t}_rows"]
        masks = np.unpackbits(z[f"f{t}_masks"], axis=-1)[:, :H * W].reshape(len(rows), H, W).astype(bool)
        frames.append(SimpleNamespace(rows=rows, masks=masks))
    return meta, inputs, frames
