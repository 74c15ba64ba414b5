"""Cases, input recipe, restatements and screens of the video panoptic post-processing tests (tests/test_panoptic_cpu.py,
tests/test_hip_panoptic.py, tools/gen_golden_panoptic.py).

`post_process` restates MaXTron_Video-kMaX/maxtron_deeplab/maxtron_cc_model.py:442-458 (`video_seg_post_processing`) and `merge`
restates :460-571 (`panoptic_mask_inference`; maxtron_wc_model.py:440-551 is the same code), op for op, in the dtype of their
inputs: run in float64 they are the reference the device is compared with, run in float32 they are the reference's own op sequence
-- the yardstick whose distance from float64 sizes the screens.  The only addition is `stable=True` in the argsort: equal reorder
scores go to the lower slot (the reference leaves ties open; slots without area all score 0 and are never accepted).

The outputs are discrete, so the cases are SCREENED instead of compared with a tolerance (`screen`): no pixel score within
`band = 8 x max |softmax_fp32 - softmax_fp64|` of the pixel threshold (8: the project's usual margin over the reference's own fp32
error, for another summation and interpolation order), every deciding class score at least 1e-4 from its threshold, reorder scores
of slots with area pairwise at least 1e-5 apart (relative), and the fp32 composition giving the float64 map exactly.  Seeds are
tried in order (`find_seed`); the seeds that pass are pinned in tests/golden/g20_panoptic_seeds.json and tests/test_panoptic_cpu.py
asserts the screens on them.
"""
import functools
import os
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# (N, T, h, w, H, W, K): mask logits [N, T, h, w], padded image H x W, K classes
CASES = [(3, 1, 4, 5, 9, 11, 4), (16, 2, 6, 10, 24, 40, 7), (20, 1, 7, 9, 25, 33, 10), (100, 3, 8, 8, 32, 32, 40), (128, 2, 9, 13, 33, 49, 124),
         (260, 1, 5, 7, 17, 20, 19), (128, 2, 45, 80, 180, 320, 124),
         # the resize SHRINKS the logits: a 16 x 16 output tile reads more than 256 low-resolution positions per slot (the staging loop's
         # other form), and with 40 slots that box no longer fits in LDS (the taps come straight from global memory)
         (16, 1, 40, 48, 20, 24, 7), (40, 1, 40, 48, 20, 24, 7)]
FIXTURE_CASES = CASES[:5]          # stored with the reference's own results (tests/golden/g20_panoptic_*.npz)
MULTI_WG = CASES[6]                # many 16 x 16 output tiles per frame
SCALES = (1.0, 0.7)                # scale_factor >= 1: crop only; < 1: crop + second resize, to a size larger than the crop
# (pixel threshold, overlap, thing class threshold, stuff class threshold, reorder class weight, reorder mask weight)
SETTINGS = [(0.4, 0.8, 0.7, 0.5, 1.0, 1.0), (0.3, 0.8, 0.2, 0.3, 1.0, 1.0), (0.3, 0.5, 0.2, 0.3, 0.5, 2.0)]
LABEL_DIVISOR = 1000
EMB = 16
SEED0 = 20000
MAX_SEEDS = 12
MAX_ROUNDS = 30
PINNED = os.path.join(GOLDEN, "g20_panoptic_seeds.json")      # per case: the first seed that passes `screen`, and its nudges (see `find_seed`)


def case_name(c):
    return "g20_panoptic_N%d_T%d_h%d_w%d_H%d_W%d_K%d" % tuple(c)


def ids_of(K):
    """contiguous class ids: the first half things, the rest stuff"""
    return list(range(K // 2)), list(range(K // 2, K))


def geometry(c, sf):
    """the arguments of video_seg_post_processing after the tensor: align_corners from the width parity (maxtron_cc_model.py:343)"""
    N, T, h, w, H, W, K = c
    ac = W % 2 == 1
    if sf >= 1:
        return SimpleNamespace(ac=ac, image_h=H, image_w=W, sf=sf, scaled_h=H - 3, scaled_w=W - 5, height=H - 2, width=W - 1)
    return SimpleNamespace(ac=ac, image_h=H, image_w=W, sf=sf, scaled_h=H - 3, scaled_w=W - 5, height=H + 5, width=W + 7)


def make_inputs(c, seed):
    """fp16-representable values.  Logits randn * 4; twin slots (copies + 0.15 randn on the upper half of every frame: two-candidate
    pixels); triplets (two copies + 0.02 .. 0.05 randn on the left half: three-candidate pixels at threshold 0.3); class logits
    randn with a label drawn from a small pool and boosted by rand * 6 (repeated stuff classes, several things per class,
    low-confidence slots)."""
    N, T, h, w, H, W, K = c
    g = torch.Generator().manual_seed(seed)
    mp = torch.randn(N, T, h, w, generator=g) * 4.0
    for i in range(0, N // 2, 2):
        mp[i + 1, :, : h // 2] = mp[i, :, : h // 2] + 0.15 * torch.randn(T, h // 2, w, generator=g)
    for i in range(N // 2, N - 2, 5):
        for j in (1, 2):
            s = 0.02 + 0.03 * float(torch.rand((), generator=g))
            mp[i + j, :, :, : (w + 1) // 2] = mp[i, :, :, : (w + 1) // 2] + s * torch.randn(T, h, (w + 1) // 2, generator=g)
    mp = mp.half().float()
    cls = torch.randn(N, K + 1, generator=g)
    pool = torch.randint(0, K, (max(3, N // 3),), generator=g)
    lab = pool[torch.randint(0, len(pool), (N,), generator=g)]
    cls[torch.arange(N), lab] += torch.rand(N, generator=g) * 6.0
    emb = torch.randn(N, EMB, generator=g)
    return mp, cls.half().float(), emb.half().float()


def post_process(mp, g):
    """maxtron_cc_model.py:442-458"""
    mp = F.interpolate(mp, size=(g.image_h, g.image_w), mode="bilinear", align_corners=g.ac)
    if g.sf < 1:
        mp = mp[:, :, :g.scaled_h, :g.scaled_w]
        mp = F.interpolate(mp, size=(g.height, g.width), mode="bilinear", align_corners=g.ac)
    else:
        mp = mp[:, :, :g.height, :g.width]
    return mp


def merge(mask_cls, mask_pred, mask_embedding, setting, thing_ids, stuff_ids, label_divisor=LABEL_DIVISOR, stats=True):
    """maxtron_cc_model.py:460-571 in the dtype and on the device of `mask_pred`.  Returns (panoptic_seg_mask, dic_cat_idemb, info):
    `info` holds what the screens and the slot-table comparisons need (`stats=False`: the reference's operations alone, nothing
    counted -- what tools/panoptic_time.py times)."""
    thr, overlap_threshold, cls_threshold_thing, cls_threshold_stuff, reorder_class_weight, reorder_mask_weight = setting
    num_mask_slots = mask_pred.shape[0]
    cls_scores, cls_labels = F.softmax(mask_cls, dim=-1)[..., :-1].max(-1)                                    # :475
    mask_scores = F.softmax(mask_pred, dim=0)
    binary_masks = mask_scores > thr
    mask_scores_flat = mask_scores.flatten(1)
    binary_masks_flat = binary_masks.flatten(1).to(mask_pred.dtype)
    pixel_number_flat = binary_masks_flat.sum(1)
    mask_scores_flat = (mask_scores_flat * binary_masks_flat).sum(1) / torch.clamp(pixel_number_flat, min=1.0)
    reorder_score = (cls_scores ** reorder_class_weight) * (mask_scores_flat ** reorder_mask_weight)         # :484
    reorder_indices = torch.argsort(reorder_score, dim=-1, descending=True, stable=True)
    all_ids = sorted(thing_ids + stuff_ids)                                                                   # :491-494
    id_cont_to_ids_dic = dict(enumerate(all_ids))
    panoptic_seg = torch.zeros(mask_pred.shape[1:], dtype=torch.int32, device=mask_pred.device)
    panoptic_seg_mask = torch.ones(mask_pred.shape[1:], dtype=torch.int32, device=mask_pred.device) * (-1)
    dic_tmp, dic_cat_idemb = {}, {}
    current_segment_id = 0
    stuff_memory_list = {}
    info = SimpleNamespace(scores=mask_scores, area=binary_masks.flatten(1).sum(1), order=reorder_indices, labels=cls_labels, cls_scores=cls_scores,
                           reorder=reorder_score, final_id=torch.full((num_mask_slots,), -1, dtype=torch.int64), things=[], rej_overlap=0,
                           rej_conf=0, merged_stuff=0, exact_tie=0, cls_margin=float("inf"))
    for i in range(num_mask_slots):                                                                           # :507-557
        cur_idx = reorder_indices[i].item()
        cur_binary_mask = binary_masks[cur_idx]
        cur_mask_embedding = mask_embedding[cur_idx]
        cur_cls_score = cls_scores[cur_idx].item()
        cur_cls_label = cls_labels[cur_idx].item()
        is_thing = cur_cls_label in thing_ids
        is_confident = (is_thing and cur_cls_score > cls_threshold_thing) or ((not is_thing) and cur_cls_score > cls_threshold_stuff)
        original_pixel_number = cur_binary_mask.to(mask_pred.dtype).sum()
        new_binary_mask = torch.logical_and(cur_binary_mask, (panoptic_seg == 0))
        new_pixel_number = new_binary_mask.to(mask_pred.dtype).sum()
        is_not_overlap_too_much = new_pixel_number > (original_pixel_number * overlap_threshold)
        if stats and original_pixel_number > 0:          # a slot without pixels is rejected whatever its class score
            info.cls_margin = min(info.cls_margin, abs(cur_cls_score - (cls_threshold_thing if is_thing else cls_threshold_stuff)))
            info.rej_conf += int(not is_confident)
            if is_confident:
                info.rej_overlap += int(not bool(is_not_overlap_too_much))
                info.exact_tie += int(float(new_pixel_number) == float(original_pixel_number) * overlap_threshold)
        if is_confident and is_not_overlap_too_much:
            cat_id_ = id_cont_to_ids_dic[int(cur_cls_label)]
            if not is_thing:
                if int(cur_cls_label) in stuff_memory_list.keys():
                    panoptic_seg[new_binary_mask] = stuff_memory_list[int(cur_cls_label)]
                    info.merged_stuff += 1
                    info.final_id[cur_idx] = cat_id_
                    continue
                else:
                    stuff_memory_list[int(cur_cls_label)] = current_segment_id + 1
            current_segment_id += 1
            panoptic_seg[new_binary_mask] = current_segment_id
            if is_thing:
                dic_tmp.setdefault((cat_id_, True), []).append((current_segment_id, cur_mask_embedding))
                ii = len(dic_tmp[(cat_id_, True)]) - 1
                info.final_id[cur_idx] = cat_id_ * label_divisor + ii
                info.things.append((cur_idx, cat_id_, ii))
            else:
                dic_tmp.setdefault((cat_id_, False), []).append(current_segment_id)
                info.final_id[cur_idx] = cat_id_
    for (cat_id_, isthing), curr_seg_id_list in dic_tmp.items():                                              # :559-569
        if isthing:
            dic_cat_idemb[cat_id_] = []
            for ii, (cur_seg_id, id_emb) in enumerate(curr_seg_id_list):
                panoptic_seg_mask[panoptic_seg == cur_seg_id] = cat_id_ * label_divisor + ii
                dic_cat_idemb[cat_id_].append(F.normalize(id_emb, p=2, dim=0))
        else:
            for cur_seg_id in curr_seg_id_list:
                panoptic_seg_mask[panoptic_seg == cur_seg_id] = cat_id_
    info.segments = current_segment_id
    return panoptic_seg_mask, dic_cat_idemb, info


def restate(c, inputs, sf, setting, dtype=torch.float64):
    mp, cls, emb = inputs
    things, stuff = ids_of(c[6])
    return merge(cls.to(dtype), post_process(mp.to(dtype), geometry(c, sf)), emb.to(dtype), setting, things, stuff)


def band_screen(c, inputs):
    """(ok, why, errors): no float64 pixel score within 8 x the fp32 composition's own error of a pixel threshold, per scale"""
    errs = []
    for sf in SCALES:
        g = geometry(c, sf)
        s64 = F.softmax(post_process(inputs[0].double(), g), dim=0)
        err = float((F.softmax(post_process(inputs[0], g), dim=0).double() - s64).abs().max())
        errs.append(err)
        for thr in sorted({t[0] for t in SETTINGS}):
            if bool(((s64 - thr).abs() <= 8.0 * err).any()):
                return False, f"sf={sf}: a pixel score within {8.0 * err:.1e} of the threshold {thr}", errs
    return True, "", errs


def screen(c, inputs):
    """(ok, why, stats): the screens of the module docstring over every scale and setting of the case; `stats` counts what the float64
    runs show (candidate multiplicities, rejections, merged stuff, the largest ii, exact overlap ties) and keeps the fp32 errors."""
    st = dict(two=0, three=0, rej_overlap=0, rej_conf=0, merged_stuff=0, max_ii=-1, exact_tie=0, err=[])
    ok, why, st["err"] = band_screen(c, inputs)
    if not ok:
        return False, why, st
    for sf in SCALES:
        for setting in SETTINGS:
            m64, d64, i64 = restate(c, inputs, sf, setting, torch.float64)
            m32, d32, i32 = restate(c, inputs, sf, setting, torch.float32)
            if i64.cls_margin < 1e-4:
                return False, f"sf={sf} {setting}: a deciding class score {i64.cls_margin:.1e} from its threshold", st
            ro = i64.reorder[i64.area > 0].sort().values
            if len(ro) > 1 and float(((ro[1:] - ro[:-1]) / ro[1:]).min()) < 1e-5:
                return False, f"sf={sf} {setting}: reorder scores closer than 1e-5", st
            if not torch.equal(m32, m64):
                return False, f"sf={sf} {setting}: the fp32 composition and float64 differ at {int((m32 != m64).sum())} pixels", st
            ncand = (i64.scores > setting[0]).sum(0)
            st["two"] += int((ncand == 2).sum())
            st["three"] += int((ncand == 3).sum())
            for k in ("rej_overlap", "rej_conf", "merged_stuff", "exact_tie"):
                st[k] += getattr(i64, k)
            st["max_ii"] = max([st["max_ii"]] + [ii for _, _, ii in i64.things])
    return True, "", st


def nudged(inputs, nudges):
    """`inputs` with 0.25 added to the low-resolution logits [n, t, r, c] listed in `nudges` (still fp16 values)"""
    mp = inputs[0].clone()
    for n, t, r, c in nudges:
        mp[n, t, r, c] += 0.25
    return (mp.half().float(),) + tuple(inputs[1:])


def _near(c, inputs):
    """(slot, frame, low-resolution row, column) nearest to every output pixel whose float64 score lies within 10x the fp32 error of
    a pixel threshold (a little wider than the screen's 8x, so that a repaired input stays clear of it)"""
    N, T, h, w, H, W, K = c
    out = set()
    for sf in SCALES:
        g = geometry(c, sf)
        s64 = F.softmax(post_process(inputs[0].double(), g), dim=0)
        err = float((F.softmax(post_process(inputs[0], g), dim=0).double() - s64).abs().max())
        bad = torch.zeros_like(s64, dtype=torch.bool)
        for thr in {t[0] for t in SETTINGS}:
            bad |= (s64 - thr).abs() <= 10.0 * err
        for n, t, y, x in bad.nonzero().tolist():
            if sf < 1:
                y, x = (y + 0.5) * g.scaled_h / g.height - 0.5, (x + 0.5) * g.scaled_w / g.width - 0.5
            r, q = (y + 0.5) * h / g.image_h - 0.5, (x + 0.5) * w / g.image_w - 0.5
            out.add((n, t, min(max(int(round(r)), 0), h - 1), min(max(int(round(q)), 0), w - 1)))
    return sorted(out)


def find_seed(c, start=0):
    """(seed offset, nudges, stats) of the first seed in start .. MAX_SEEDS - 1 that passes `screen`.  With 10^5 output pixels no seed
    keeps every score outside the band by chance (the large case has about a hundred pixels inside it at scale_factor 0.7, where the
    fp32 resize itself is 2e-5 off), so each seed's logits are first REPAIRED: while a pixel score lies near a threshold, the nearest
    low-resolution logit of that slot is raised by 0.25 (which moves the score by about 1e-2) -- up to MAX_ROUNDS rounds.  The screens
    are then applied unchanged to the repaired inputs."""
    why = []
    for s in range(start, MAX_SEEDS):
        base, nudges = make_inputs(c, SEED0 + s), []
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
    """(seed offset, nudges) of the case, as tools/gen_golden_panoptic.py found and stored them"""
    import json
    with open(PINNED) as f:
        p = json.load(f)[case_name(c)]
    return p["seed"], [tuple(x) for x in p["nudges"]]


@functools.lru_cache(maxsize=None)
def inputs_of(c):
    """the case's inputs at its pinned seed: (mask_pred [N,T,h,w], mask_cls [N,K+1], mask_embedding [N,EMB]), fp32 holding fp16 values"""
    seed, nudges = pinned(c)
    return nudged(make_inputs(c, SEED0 + seed), nudges)


@functools.lru_cache(maxsize=None)
def restated(c, sf, setting):
    """float64 restatement of the case, computed once and shared: (map int32 [T,H,W], dict, info).  Do not modify."""
    return restate(c, inputs_of(c), sf, setting)


def load_fixture(c):
    """the reference's own results: (inputs, {(sf, setting index): (map int32, [category ids in dict order], [embeddings per category])})"""
    import json
    z = np.load(os.path.join(GOLDEN, case_name(c) + ".npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    inputs = tuple(torch.from_numpy(z[k].astype(np.float32)) for k in ("mask_pred", "mask_cls", "mask_embedding"))
    out = {}
    for si, sf in enumerate(SCALES):
        for ti in range(len(SETTINGS)):
            k = f"s{si}_t{ti}"
            keys = [int(x) for x in z[k + "_keys"]]
            counts = [int(x) for x in z[k + "_counts"]]
            embs, o = [], 0
            for n in counts:
                embs.append(torch.from_numpy(z[k + "_embs"][o:o + n]))
                o += n
            out[(sf, ti)] = (torch.from_numpy(z[k + "_map"]), keys, embs)
    return meta, inputs, out
