"""Golden vectors for Tube-Link's point-sampled training loss: tests/golden/g22_tl_loss_<case>.npz and g22_tl_loss_seeds.json.

Runs on the CPU in fp32 the REFERENCE'S OWN `Mask2FormerVideoCCHeadTube.loss` / `loss_single` / `get_targets` / `_get_target_single`,
`MaskHungarianAssigner`, `MaskPseudoSampler`, `ClassificationCost` / `CrossEntropyLossCost` / `DiceCost`, `CrossEntropyLoss`, `DiceLoss`
and `get_uncertain_point_coords_with_randomness`, loaded by file path from the reference tree (build container only; the reference
never travels and none of its text is copied here).  Packages those files import but this path never needs (mmcv, the registries) are
stand-in modules; `mmcv.ops.point_sample` is its definition, F.grid_sample(input, 2 p - 1, align_corners=False).  torch.rand is wrapped
to record every draw, SciPy's linear_sum_assignment to record the cost it is given, torch.topk to record the kept candidates.

    python tools/gen_golden_tl_loss.py [reference root]      # default: the checkout oracle/gen_golden_tl.py names

A fixture holds what the reference computed -- the draws (shape and SHA-256 each: the inputs and the coordinates are regenerated from
the case's seed by tests/tl_loss_cases.py), the assignments, the costs, the kept candidates, the three losses per layer and the
gradients of sum_i w_i loss_i (tl_loss_cases.upstream_weights) -- and no input.  The seeds are the first that pass the screens of
tests/tl_loss_cases.py."""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import gen_golden_tl as gt  # noqa: E402
import tl_loss_cases as tc  # noqa: E402

TL = sys.argv[1] if len(sys.argv) > 1 else gt.TL


def _mod(name, **kw):
    m = types.ModuleType(name)
    m.__dict__.update(kw)
    m.__path__ = []
    sys.modules[name] = m
    return m


def _load(dotted, path=None):
    path = path or f"{TL}/{dotted.replace('.', '/')}.py"
    spec = importlib.util.spec_from_file_location(dotted, path)
    m = importlib.util.module_from_spec(spec)
    sys.modules[dotted] = m
    spec.loader.exec_module(m)
    return m


class _Registry:
    """register_module() keeps the class under its name; build(cfg) calls it with the other keys"""

    def __init__(self):
        self.classes = {}

    def register_module(self, *a, **k):
        def deco(cls):
            self.classes[cls.__name__] = cls
            return cls
        return deco

    def build(self, cfg, **kw):
        cfg = dict(cfg)
        return self.classes[cfg.pop("type")](**cfg, **kw)


def point_sample(input, points, align_corners=False, **kwargs):
    """mmcv.ops.point_sample: F.grid_sample at 2 p - 1"""
    add_dim = points.dim() == 3
    if add_dim:
        points = points.unsqueeze(2)
    out = F.grid_sample(input, 2.0 * points - 1.0, align_corners=align_corners, **kwargs)
    return out.squeeze(3) if add_dim else out


def load_reference():
    ident = lambda *a, **k: (lambda f: f)
    costs, assigners, samplers, losses = _Registry(), _Registry(), _Registry(), _Registry()
    _mod("mmcv", jit=ident)
    _mod("mmcv.cnn", Conv2d=torch.nn.Conv2d, build_plugin_layer=None, caffe2_xavier_init=None)
    _mod("mmcv.cnn.bricks")
    _mod("mmcv.cnn.bricks.transformer", build_positional_encoding=None, build_transformer_layer_sequence=None)
    _mod("mmcv.ops", point_sample=point_sample)
    _mod("mmcv.runner", ModuleList=torch.nn.ModuleList, force_fp32=ident, auto_fp16=ident)
    _mod("mmdet")
    _mod("mmdet.utils")
    _load("mmdet.utils.util_mixins")
    sys.modules["mmdet.utils"].util_mixins = sys.modules["mmdet.utils.util_mixins"]
    _mod("mmdet.core", build_assigner=assigners.build, build_sampler=samplers.build, reduce_mean=lambda t: t,
         multi_apply=lambda func, *args: tuple(map(list, zip(*map(func, *args)))))
    _mod("mmdet.core.bbox")
    _mod("mmdet.core.bbox.builder", BBOX_ASSIGNERS=assigners, BBOX_SAMPLERS=samplers)
    _mod("mmdet.core.bbox.iou_calculators", bbox_overlaps=None)
    _mod("mmdet.core.bbox.transforms", bbox_cxcywh_to_xyxy=None, bbox_xyxy_to_cxcywh=None)
    _mod("mmdet.core.bbox.match_costs")
    _mod("mmdet.core.bbox.match_costs.builder", MATCH_COST=costs, build_match_cost=costs.build)
    _load("mmdet.core.bbox.match_costs.match_cost")
    _mod("mmdet.core.bbox.assigners")
    for n in ("assign_result", "base_assigner", "mask_hungarian_assigner"):
        _load("mmdet.core.bbox.assigners." + n)
    _mod("mmdet.core.bbox.samplers")
    for n in ("sampling_result", "base_sampler", "mask_sampling_result", "mask_pseudo_sampler"):
        _load("mmdet.core.bbox.samplers." + n)
    _mod("mmdet.models")
    _mod("mmdet.models.builder", HEADS=_Registry(), LOSSES=losses, build_loss=losses.build)
    _mod("mmdet.models.losses")
    for n in ("utils", "cross_entropy_loss", "dice_loss"):
        _load("mmdet.models.losses." + n)
    _mod("mmdet.models.utils")
    ps = _load("mmdet.models.utils.point_sample")
    sys.modules["mmdet.models.utils"].get_uncertain_point_coords_with_randomness = ps.get_uncertain_point_coords_with_randomness
    _mod("mmdet.models.dense_heads")
    _mod("mmdet.models.dense_heads.anchor_free_head", AnchorFreeHead=torch.nn.Module)
    for p in ["models", "models.video", "models.video.tube_link_vps", "models.video.tube_link_vis"]:
        _mod(p)
    _mod("models.video.tube_link_vps.utils", preprocess_video_panoptic_gt=None)
    _mod("models.video.tube_link_vis.memory", retry_if_cuda_oom=None)
    if "timm.models.layers" not in sys.modules:
        _mod("timm"); _mod("timm.models")
        _mod("timm.models.layers", trunc_normal_tf_=torch.nn.init.trunc_normal_)
    head = _load("tl_cc_head", f"{TL}/models/video/tube_link_vis/mask2former_video_cc_head.py")
    return head, assigners, samplers, losses


def harness(head_mod, assigners, samplers, losses, c, class_weight):
    Head = head_mod.Mask2FormerVideoCCHeadTube

    class Harness:
        loss = Head.loss
        loss_single = Head.loss_single
        get_targets = Head.get_targets
        _get_target_single = Head._get_target_single

    hs = Harness()
    hs.num_classes = c["K"]
    hs.class_weight = class_weight
    hs.point_loss = True
    hs.num_points, hs.oversample_ratio, hs.importance_sample_ratio = c["P"], c["over"], c["ratio"]
    hs.assigner = assigners.build(dict(type="MaskHungarianAssigner", cls_cost=dict(type="ClassificationCost", weight=tc.COST_W[0]),
                                       mask_cost=dict(type="CrossEntropyLossCost", weight=tc.COST_W[1], use_sigmoid=True),
                                       dice_cost=dict(type="DiceCost", weight=tc.COST_W[2], pred_act=True, eps=tc.DICE_EPS)))
    hs.sampler = samplers.build(dict(type="MaskPseudoSampler"), context=hs)
    hs.loss_cls = losses.build(dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=tc.LOSS_W[0], reduction="mean", class_weight=class_weight))
    hs.loss_mask = losses.build(dict(type="CrossEntropyLoss", use_sigmoid=True, reduction="mean", loss_weight=tc.LOSS_W[1]))
    hs.loss_dice = losses.build(dict(type="DiceLoss", use_sigmoid=True, activate=True, reduction="mean", naive_dice=True, eps=tc.DICE_EPS,
                                     loss_weight=tc.LOSS_W[2]))
    return hs


def run_reference(ref, c, seed):
    head_mod, assigners, samplers, losses = ref
    inp = tc.make_inputs(c, seed)
    hs = harness(head_mod, assigners, samplers, losses, c, [float(x) for x in inp["class_weight"]])
    cls = [t.clone().requires_grad_(True) for t in inp["cls"]]
    mps = [t.clone().requires_grad_(True) for t in inp["masks"]]
    want = tc.draw(c, seed)                       # the package's draws (hand-placed where the case says so): must be what torch.rand gives
    asg = sys.modules["mmdet.core.bbox.assigners.mask_hungarian_assigner"]
    draws, lsa, kept = [], [], []
    real_rand, real_lsa, real_topk = torch.rand, asg.linear_sum_assignment, torch.topk
    S, k, G = tc.counts(c)
    B = len(c["M"])
    per_layer = B + (0 if G == 0 else (1 if c["P"] - k == 0 else 2))

    def rand(*a, **kw):
        out = real_rand(*a, **kw)
        i = len(draws)
        draws.append(out.clone())
        if c.get("hand"):                         # hand-placed coordinates take the place of the draw they overwrite
            l, j = divmod(i, per_layer)
            out = want[0][l, j][None] if j < B else (want[1][l] if j == B else want[2][l])
            assert out.shape == draws[-1].shape
        return out

    def lsa_rec(cost):
        r = real_lsa(cost)
        lsa.append((np.asarray(cost, dtype=np.float32).copy(), np.asarray(r[0]).copy(), np.asarray(r[1]).copy()))
        return r

    def topk(*a, **kw):
        r = real_topk(*a, **kw)
        kept.append(r[1].clone())
        return r

    torch.manual_seed(seed + 1)
    torch.rand, asg.linear_sum_assignment, torch.topk = rand, lsa_rec, topk
    try:
        out = hs.loss(cls, mps, inp["labels"], inp["gt"], [None] * B)
    finally:
        torch.rand, asg.linear_sum_assignment, torch.topk = real_rand, real_lsa, real_topk
    L = c["L"]
    assert list(out) == tc.loss_keys(L)
    flat = torch.stack([out[k_].reshape(()) for k_ in tc.loss_keys(L)])
    ref_losses = torch.zeros(3 * L)
    ref_losses[tc.layer_of_key(L)] = flat.detach()
    w = torch.tensor(tc.upstream_weights(L), dtype=torch.float32)
    (ref_losses.new_tensor(0.0) + sum(w[pos] * out[k_] for k_, pos in zip(tc.loss_keys(L), tc.layer_of_key(L)))).backward()
    return dict(inp=inp, draws=draws, lsa=lsa, kept=kept, losses=ref_losses.reshape(L, 3), dcls=[t.grad if t.grad is not None else torch.zeros_like(t) for t in cls],
                dmasks=[t.grad if t.grad is not None else torch.zeros_like(t) for t in mps])


def main():
    ref = load_reference()
    seeds = {}
    for name, c in tc.CASES.items():
        seed = tc.find_seed(c)
        seeds[name] = seed
        r = run_reference(ref, c, seed)
        L, B = c["L"], len(c["M"])
        S, k, G = tc.counts(c)
        arrays = {}
        it = iter(r["lsa"])
        for l in range(L):
            for b, M in enumerate(c["M"]):
                if M > 0:
                    cost, rows, cols = next(it)
                    arrays[f"cost_{l}_{b}"] = cost
                else:
                    rows = cols = np.zeros(0, dtype=np.int64)
                arrays[f"rows_{l}_{b}"], arrays[f"cols_{l}_{b}"] = rows.astype(np.int64), cols.astype(np.int64)
            if name not in tc.BIG:
                arrays[f"sel_{l}"] = (np.sort(r["kept"][l].numpy(), axis=1) if G > 0 else np.zeros((0, k))).astype(np.uint16)
            arrays[f"ref_dcls_{l}"] = r["dcls"][l].numpy()
            dm = r["dmasks"][l]
            arrays[f"ref_dmasks_{l}"] = (dm.reshape(-1)[::tc.DMASK_STRIDE] if name in tc.BIG else dm).numpy()
        arrays["ref_losses"] = r["losses"].numpy()
        meta = dict(case=name, seed=seed, torch=torch.__version__, draws=[dict(shape=list(d.shape), sha256=tc.digest(d)) for d in r["draws"]])
        arrays["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
        path = os.path.join(tc.GOLDEN, f"g22_tl_loss_{name}.npz")
        np.savez_compressed(path, **arrays)
        print(f"{name}: seed {seed}, {len(r['draws'])} draws, {os.path.getsize(path)} bytes, losses {r['losses'].reshape(-1).tolist()}")
    with open(tc.SEEDS_FILE, "w") as f:
        json.dump(seeds, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
