"""The cross-clip tracking module's training tier (axvs_cc_train.h, axvs_cc_train_host.h, cc_training.py) off its fixture grid: the case
table, weights, inputs, float64 reference and error measures shared by tests/test_cc_train_cases_cpu.py and
tests/test_hip_cc_training.py.

REFERENCE.  oracle/axvs_oracle.py::cc_module_train in float64 under torch.autograd (held to the reference implementation by
tests/test_oracle_golden.py; it takes any shape).  The same function in float32 is the yardstick of the ratio r below.

WEIGHTS.  orc.random_weights over orc.cc_module_param_shapes, then the running_mean of the four BatchNorm sites overwritten with values
of magnitude 0.25 .. 1.5 and random sign.  The statistics kernels subtract the running mean before they sum (the shift), so a row, column
or element counted wrongly in a tail moves a batch mean by a fraction of the shift; with random_weights' own U(-0.1, 0.1) that fraction
can hide under the tolerance.

INPUTS.  clip_query ~ N(0, 1) [B, Q, Tc, 256], panoptic_features normalised over its 128 channels, d_logits ~ N(0, 1) per layer,
d_masks ~ 0.01 N(0, 1) per layer: the recipe of test_cc_training_at_baseline_config_4_vs_float64_oracle.

ERROR MEASURES (those of test_hip_cc_training.py).  An output, d_clip_query, a batch variance: max|got - ref| / max|ref| (rel_err) and, for
the outputs and d_clip_query, |got - ref|_2 / |ref|_2 (rel_l2).  A parameter gradient: |got - ref|_2 / max(|ref|_2, 1e-3 * the largest
gradient norm of the module).  A batch mean: max|got - ref| / max(max|mean|, sqrt(max var)): a mean serves only in (x - mean) / std, so
its error counts against the data's scale.  By construction the pixel-space site's one mean is 1e-4 .. 1e-2 of its std here, and an
error of one ulp of the shift, 1e-7, would already be 1e-4 .. 1e-3 of such a mean.  A running buffer after the step: rel_err against
the oracle's batch statistics pushed through the module's momentum update (momentum 0.01, one step per layer).

BATCH STATISTICS PER LAYER.  With momentum 0.01 a buffer is 0.99^L of what it was plus a hundredth of the statistics, so the buffer
comparison sees a hundredth of an error in them.  The module hands the statistics out only through its buffers, and a buffer after a step
with momentum m is (1 - m)^L r0 + sum_l m (1 - m)^(L-1-l) s_l (m = None: the mean of the s_l from a fresh counter).  L forwards with the
momenta STAT_MOMENTA[:L] = 1 (the last layer alone), None, 0.5 give L independent combinations, and `layer_stats` solves them for the
s_l in float64.  The solve multiplies the fp32 rounding of the buffers by at most the largest absolute row sum of the inverse of that
L x L system (`stat_solve_amplification`): 1, 3 and 16 for L = 1, 2, 3 (L = 3: the inverse is [[2, 6, -8], [-3, -3, 8], [1, 0, 0]]),
so 16 * 2^-24 = 1e-6 of the buffers' scale against TOL = 1e-4; the CPU test asserts these figures.

THE RATIO r of a tensor = max|device - f64| / max(max|oracle fp32 - f64|, 2^-24 max|f64|): how far the device is from float64 in units
of what plain fp32 torch is; the floor is one rounding of an fp32 result.  It is taken over the outputs, d_clip_query and the parameter
gradients, not over the recovered statistics, whose error holds the buffers' rounding through the solve besides the kernels' own.

WHAT EACH CASE REACHES is derived from the host code next to it in CASES; `structure` restates those host formulas (cc_forward's
fused-statistics condition and tile counts, dk_plan, cc_scalar_stats' block plan) and the CPU test asserts each claim, so the table cannot
drift from its comments.  kGT = 128 is the GEMM tile, kGK = 32 its contraction step."""
import math
from collections import namedtuple

import torch

import axvs_oracle as orc
from golden_util import rel_err, rel_l2

TOL = 1e-4          # the bar of test_hip_cc_training.py
FLOOR = 2.0 ** -24
MOMENTUM = 0.01     # the module's BatchNorm momentum
STAT_MOMENTA = (1.0, None, 0.5)     # one forward each recovers the batch statistics of up to three layers (layer_stats)
KGT, KGK = 128, 32
BN_SITES = ("_class_embedding_projection.norm", "_mask_embedding_projection.norm", "_predictor._transformer_mask_head.norm",
            "_predictor._pixel_space_mask_batch_norm")

Case = namedtuple("Case", "B Q Tc V H W layers K1 rates p_attn_drop p_aspp_drop seed")

CASES = {
    # B == 1, Q % 128 == 0: fused statistics.  P = 135 = 128 + 7: tiles_p = 2, the second pixel tile has 7 live columns; rows of P floats
    # start at odd offsets (row_align 4 bytes).  Tc = 2: stat_blk0 = 0, 2.  dk_plan: nk = ceil(135 / 32) = 5, rows = 2 * 128 -> mt = 2,
    # want = 256, ks = max(4, 1) = 4, z = 2: the last split is the one k-step of 7 columns.  E = 34560: backward cc_scalar_stats, 3 blocks
    "fused_ragged": Case(1, 128, 2, 1, 9, 15, 2, 5, (1, 2, 3), 0.0, 0.0, 4101),
    # qtiles = 2: tile = pixel tile + tiles_p * query tile, stat_blk0 = t * 4 over three clips; P = 130; K1 = 134 = 4 * 33 + 2
    "fused_two_qtiles": Case(1, 256, 3, 2, 5, 13, 1, 134, (1, 2, 3), 0.0, 0.0, 4102),
    # Tc = 1: softmax over one entry, every ASPP tap clamps to the row itself, attention over T = 1; P = 128 whole tile, aligned rows;
    # K1 = 2: log(K1 - 1) = 0 in the void bias
    "fused_tc1": Case(1, 128, 1, 1, 8, 16, 1, 2, (1, 2, 3), 0.0, 0.0, 4103),
    # Tc = 16, the stated maximum (make_cc_shape refuses 17); Q = 8 the smallest; P = 21 odd; three layers; both dropouts on
    "plain_tc16": Case(1, 8, 16, 1, 3, 7, 3, 5, (1, 2, 3), 0.1, 0.1, 4104),
    # Tc = 2 with rates (1, 2, 3): rates 2 and 3 >= Tc, both outer taps of those branches clamp for every t
    "plain_rate_over_tc": Case(1, 16, 2, 1, 4, 5, 2, 5, (1, 2, 3), 0.0, 0.0, 4105),
    # the same with rates (6, 12, 18): every outer tap of every branch clamps (the gather of cct_col2im_add_kernel)
    "plain_rate_over_tc_6_12_18": Case(1, 16, 2, 1, 4, 5, 2, 5, (6, 12, 18), 0.0, 0.0, 4105),
    # Q = 136 = 128 + 8: a whole query tile plus 8 rows, Q % 128 != 0 so not fused; P = 33 odd
    "plain_q136": Case(1, 136, 2, 1, 3, 11, 1, 5, (1, 2, 3), 0.0, 0.0, 4106),
    # E = 40 * 4 * 301 = 48160 > 2 * 16384: cc_scalar_stats with 3 blocks of 16056, the last one 16048; P = 301 odd: nk = 10, ks = 4, z = 3
    "plain_scalar_blocks": Case(1, 40, 4, 1, 7, 43, 1, 5, (1, 2, 3), 0.0, 0.0, 4107),
    # B = 2: the per-(layer, video, clip) GEMM loops, cct_scalar_bn_bwd_apply_kernel writes dpre; P = 300: nk = 10, ks = 4, z = 3 with a
    # last split of 2 steps, the second of 12 columns; E = 28800: 2 blocks
    "batch2_ragged": Case(2, 16, 3, 1, 15, 20, 2, 5, (1, 2, 3), 0.0, 0.0, 4108),
    # B * Tc = 15 softmax entries per query: each of the four waves of cct_act_pool_* takes a second, third and (three of them) fourth
    # entry; P = 30, rows 8-byte aligned only; both dropouts on
    "batch3_pool": Case(3, 8, 5, 2, 3, 5, 2, 5, (1, 2, 3), 0.1, 0.1, 4109),
}
TWICE = ("fused_ragged", "batch2_ragged")      # run twice on the device, identical bits required (fixed summation orders)

# what the comments above claim, per case: the CPU test compares this with structure(case)
CLAIMS = {
    "fused_ragged": dict(fused=True, P=135, p_mod=7, tiles_p=2, qtiles=1, nk=5, ks=4, z=2, last_split_cols=7, scalar_blocks=3, entries=2),
    "fused_two_qtiles": dict(fused=True, P=130, p_mod=2, tiles_p=2, qtiles=2, nk=5, z=2, entries=3, k1_mod4=2),
    "fused_tc1": dict(fused=True, P=128, p_mod=0, tiles_p=1, qtiles=1, nk=4, z=1, entries=1, K1=2, rates_ge_tc=3),
    "plain_tc16": dict(fused=False, P=21, entries=16, layers=3, rates_ge_tc=0),
    "plain_rate_over_tc": dict(fused=False, P=20, rates_ge_tc=2, z=1, scalar_blocks=1),
    "plain_rate_over_tc_6_12_18": dict(fused=False, P=20, rates_ge_tc=3),
    "plain_q136": dict(fused=False, P=33, q_mod=8, nk=2, z=1),
    "plain_scalar_blocks": dict(fused=False, P=301, E=48160, scalar_blocks=3, scalar_per_block=16056, scalar_last_block=16048, nk=10, ks=4, z=3),
    "batch2_ragged": dict(fused=False, B=2, P=300, nk=10, ks=4, z=3, last_split_cols=44, E=28800, scalar_blocks=2),
    "batch3_pool": dict(fused=False, B=3, P=30, p_mod=30, entries=15),
}


def structure(c):
    """The host's branch and plan arithmetic for a case, restated: cc_forward (fused statistics), dk_plan, cc_scalar_stats."""
    P = c.V * c.H * c.W
    E = c.B * c.Q * c.Tc * P
    tiles_p, qtiles = -(-P // KGT), c.Q // KGT
    nk = -(-P // KGK)
    rows = c.layers * c.Q if c.B == 1 else c.Q
    want = min(max(1024 // max(-(-rows // KGT), 1), 1), 256)
    ks = max(-(-nk // want), 4)
    z = -(-nk // ks)
    nblk = min(-(-E // 16384), 1024)
    per = (-(-E // nblk) + 3) // 4 * 4
    nblk = -(-E // per)
    return dict(B=c.B, P=P, E=E, K1=c.K1, layers=c.layers, p_mod=P % KGT, q_mod=c.Q % KGT, k1_mod4=c.K1 % 4, tiles_p=tiles_p, qtiles=qtiles,
                fused=c.B == 1 and c.Q % KGT == 0 and c.Tc * tiles_p * qtiles <= 256 * 256, nk=nk, ks=ks, z=z,
                last_split_cols=P - (z - 1) * ks * KGK, scalar_blocks=nblk, scalar_per_block=per, scalar_last_block=E - (nblk - 1) * per,
                entries=c.B * c.Tc, rates_ge_tc=sum(r >= c.Tc for r in c.rates))


def make_weights(c):
    """random_weights with the four running means of order 1 (no zeros)"""
    w = orc.random_weights(orc.cc_module_param_shapes(c.layers, c.K1 - 1), c.seed)
    g = torch.Generator().manual_seed(c.seed + 7)
    for site in BN_SITES:
        n = w[site + ".running_mean"].numel()
        mag = 0.25 + 1.25 * torch.rand(n, generator=g)
        sign = (torch.rand(n, generator=g) < 0.5).float() * 2 - 1
        w[site + ".running_mean"] = mag * sign
    return w


def make_inputs(c):
    """(clip_query, panoptic_features, d_logits per layer, d_masks per layer), fp32"""
    g = torch.Generator().manual_seed(c.seed + 1)
    cq = torch.randn(c.B, c.Q, c.Tc, 256, generator=g)
    pf = torch.nn.functional.normalize(torch.randn(c.B, 128, c.Tc * c.V, c.H, c.W, generator=g), dim=1)
    d_logits = [torch.randn(1, c.Q, c.K1, generator=g) for _ in range(c.layers)]
    d_masks = [torch.randn(c.B, c.Q, c.Tc * c.V, c.H, c.W, generator=g) * 0.01 for _ in range(c.layers)]
    return cq, pf, d_logits, d_masks


_refs = {}


def reference(case, dtype=torch.float64):
    """One training step of the oracle in `dtype` -> dict: logits [L, 1, Q, K1], masks [L, B, Q, Tc V, H, W], d_clip_query, grads {name:
    tensor}, stats {site: (mean [L, C], unbiased var [L, C])}.  Computed once per (case, dtype) and shared: leave it unchanged."""
    key = (case, dtype)
    if key not in _refs:
        c = CASES[case]
        w = make_weights(c)
        cq, pf, d_logits, d_masks = make_inputs(c)
        wd = {k: v.to(dtype).requires_grad_("running" not in k) for k, v in w.items()}
        q = cq.to(dtype).requires_grad_(True)
        logits, masks, stats = orc.cc_module_train(q, pf.to(dtype), wd, c.layers, c.V, list(c.rates), c.p_attn_drop, c.p_aspp_drop, c.seed)
        loss = sum((a * b.to(dtype)).sum() for a, b in zip(logits, d_logits)) + sum((a * b.to(dtype)).sum() for a, b in zip(masks, d_masks))
        loss.backward()
        _refs[key] = dict(logits=torch.stack([x.detach() for x in logits]), masks=torch.stack([x.detach() for x in masks]), d_clip_query=q.grad,
                          grads={k: v.grad for k, v in wd.items() if v.requires_grad},
                          stats={s: (torch.stack([m for m, _ in stats[s]]), torch.stack([v for _, v in stats[s]])) for s in BN_SITES})
    return _refs[key]


def running_after(case, ref):
    """{buffer name: value after one training step}: the reference's statistics through the module's update, one momentum step per
    layer in layer order; num_batches_tracked counts the layers"""
    c = CASES[case]
    w = make_weights(c)
    out = {}
    for s in BN_SITES:
        for j, kind in enumerate(("running_mean", "running_var")):
            r = w[f"{s}.{kind}"].double()
            for l in range(c.layers):
                r = (1 - MOMENTUM) * r + MOMENTUM * ref["stats"][s][j][l].double()
            out[f"{s}.{kind}"] = r
        out[s + ".num_batches_tracked"] = c.layers
    return out


def momentum_weights(m, L):
    """(c, [w_l]): a buffer after one step of L layers with momentum m is c r0 + sum_l w_l s_l (cc_training.cc_module_train)"""
    if m is None:
        return 0.0, [1.0 / L] * L
    return (1 - m) ** L, [m * (1 - m) ** (L - 1 - l) for l in range(L)]


def stat_solve_amplification(L):
    """the largest absolute row sum of the inverse of layer_stats' system for L layers: an error of e in every buffer becomes at most
    this times e in a recovered statistic"""
    A = torch.tensor([momentum_weights(m, L)[1] for m in STAT_MOMENTA[:L]], dtype=torch.float64)
    return float(torch.linalg.inv(A).abs().sum(1).max())


def layer_stats(case, buffers):
    """The batch statistics of every layer from the buffers after one step with each of STAT_MOMENTA[:L] (buffers[j]: {name: tensor})
    -> {site: (mean [L, C], unbiased var [L, C])}, float64"""
    c = CASES[case]
    L = c.layers
    assert L <= len(STAT_MOMENTA) == len(set(STAT_MOMENTA)) and len(buffers) == L
    w0 = make_weights(c)
    cw = [momentum_weights(m, L) for m in STAT_MOMENTA[:L]]
    A = torch.tensor([w for _, w in cw], dtype=torch.float64)
    out = {}
    for s in BN_SITES:
        both = []
        for kind in ("running_mean", "running_var"):
            rhs = torch.stack([buffers[j][f"{s}.{kind}"].double().cpu() - cw[j][0] * w0[f"{s}.{kind}"].double() for j in range(L)])
            both.append(torch.linalg.solve(A, rhs))
        out[s] = tuple(both)
    return out


def tensors(res):
    """the flat {label: tensor} view of a result dict ('stats' optional)"""
    out = dict(logits=res["logits"], masks=res["masks"], d_clip_query=res["d_clip_query"])
    out.update({"grad." + k: v for k, v in res["grads"].items()})
    for s, (m, v) in res.get("stats", {}).items():
        out[f"stat.{s}.mean"], out[f"stat.{s}.var"] = m, v
    return out


def errors(got, ref):
    """every measure of `got` (a result dict; 'stats' optional) against `ref` -> {label: error}, each to be held under TOL"""
    e = {}
    for k in ("logits", "masks", "d_clip_query"):
        e[k] = rel_err(got[k], ref[k])
        e[k + "_l2"] = rel_l2(got[k], ref[k])
    floor = 1e-3 * max(float(v.norm()) for v in ref["grads"].values())
    for k, v in ref["grads"].items():
        e["grad." + k] = float((got["grads"][k].double() - v.double()).norm() / max(float(v.double().norm()), floor))
    for s, (m, v) in got.get("stats", {}).items():
        rm, rv = ref["stats"][s]
        e[f"stat.{s}.mean"] = float((m.double() - rm.double()).abs().max() / max(float(rm.abs().max()), float(rv.abs().max()) ** 0.5))
        e[f"stat.{s}.var"] = rel_err(v, ref["stats"][s][1])
    return e


def ratios(got, ref64, ref32):
    """per output, d_clip_query and gradient: (r, max|got - f64|, yard), r = max|got - f64| / yard, yard = max(max|fp32 oracle - f64|,
    2^-24 max|f64|);
    a tensor that is exactly zero in float64 (yard 0) has r = 0 when the device has an exact zero too, else inf"""
    g, a, b = tensors(got), tensors(ref64), tensors(ref32)
    out = {}
    for k in g:
        if k.startswith("stat."):
            continue
        x = a[k].double()
        yard = max(float((b[k].double() - x).abs().max()), FLOOR * float(x.abs().max()))
        dev = float((g[k].double().cpu() - x).abs().max())
        out[k] = ((dev / yard if yard > 0 else (0.0 if dev == 0 else math.inf)), dev, yard)
    return out


def all_finite(res):
    return all(bool(torch.isfinite(v).all()) for v in tensors(res).values())
