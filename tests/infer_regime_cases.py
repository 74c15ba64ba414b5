"""The inference tier's trajectory kernels (axvs_fused.h, axvs_attn.h, axvs_misc.h, axvs_cc.h) off the soft-softmax regime of
orc.synthetic_clip / orc.random_weights: large logits and almost one-hot softmaxes.  Shared by tests/test_infer_regimes_cpu.py and
tests/test_hip_infer_regimes.py.

CASES are cases of infer_plan_cases.CASES by name: shapes, inputs, the runner and the recorded stage names (which assert the kernel
form that ran) are that file's.  A REGIME changes only parameters, in the form of traj_train_regime_cases.regime_weights, so the modules
still load with strict=True:

  shift    k.bias * mk and the K half of proj_kv.bias * mt, per pass.  In exact arithmetic nothing but the logits' common part moves.
           On the fused forms the temporal shift never reaches the kernel's arithmetic (the K half of proj_kv.bias is dropped because it
           cancels): there the regime bites through the spatial half alone; on the generic form k2 carries its bias in fp32.
  sharp_s  q.weight and q.bias * gs.
  sharp_t  proj_q.weight and proj_q.bias * gt.
The cross-clip cases take the multipliers on the same rows of qkv.weight / qkv.bias.

YARDSTICK.  This tier rounds operands to fp16 at about 16 sites, and an fp16 logit of magnitude s is off by about s * 2^-11: off the soft
regime no fixed tolerance against float64 holds.  The yardstick is tests/f16_sites.py, the layer with exactly the kernels' roundings,
run in float64 with the sites of the kernel form that the case's recorded stages name.

SCREENING (CPU only).  PAIRS stores per (case, regime) the multipliers and a weight-seed offset, counted from infer_plan_cases.SEED: the
first ladder rung and the first of SEEDS offsets at which `screen` holds -- the regime's logit conditions (LOGIT of the training file)
on the float64 oracle, the coverage conditions (`coverage_misses`: which keys, 16-key tiles, 256-key chunks and frames take the weight)
and a yardstick that cannot hide a failure: its own distance from float64 at most YARD_CAP.  (shift has two multipliers: per offset, each
takes the first rung at which its half's largest |s| reaches the condition.)  The rung is as low as the logit conditions allow except on
the two chunked cases under sharp_s, where the jump into the last key chunk sets it (gs = 32; at 24 no seed has one).  `python
tests/infer_regime_cases.py [case | regime ...]` reruns the search.  LEFT_OUT names the pairs that cannot meet all three, with the reason.

BOUNDS.  `missed` holds a device result to max(1e-3, YARD_FACTOR * y) per output tensor, y the yardstick's largest distance from
float64 over YARD_SEEDS weight seeds of the pair at its multipliers.  YARD_FACTOR = 2 covers what the yardstick does not model: the
hardware's exp2 / rcp at 1 ulp, the MFMA's summation order, roundings that flip between two equally valid orders.
"""
import contextlib
import os
import sys

import torch

if __name__ == "__main__":      # run as a script: the oracle and the package lie next to tests/
    sys.path[:0] = [os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", d) for d in ("oracle", "")]

import axvs_oracle as orc
import f16_sites as fs
import infer_plan_cases as ipc
import traj_train_regime_cases as trc
from golden_util import rel_err, rel_l2
from traj_train_regime_cases import LOGIT, LADDER, EXP_UNDERFLOW, WRONG, Pair, REGIMES, _spatial_figures, _temporal_figures  # noqa: F401

assert (trc.K_TILE, trc.K_CHUNK) == (16, 256)          # this tier's key tiles and the long kernel's key chunks are the training tier's
TOL_F16 = 1e-3                      # the bar of test_hip_parity.py and test_hip_infer_plan.py, at ordinary inputs
TOL_MAP = 3e-3                      # ... for the spatial maps
YARD_CAP = 5e-2
YARD_FACTOR = 2.0
YARD_SEEDS = 4
SEEDS = 16
HEADS = 8

# case -> what it is there to reach (the kernel form is asserted by ipc.STAGES[case])
CASES = {
    "mq2_ffn_rides": "traj_fused, 64-row tiles, a tile is a frame, 64 keys, the FFN rides",
    "mq1_frames_32_48": "traj_fused, frames of 32 and 48 keys",
    "first_on_64_rows": "traj_fused, frames padded 40 -> 48 and 52 -> 64",
    "rows16_merged": "traj_fused on 16-row tiles, L = 16: half a key step is padding",
    "rows16_ragged": "traj_fused, 25 / 43 keys: masked keys in the last key tile",
    "rows32_merged_split2": "traj_fused on 32-row tiles, T = 5",
    "t9_rows16": "traj_fused, T = 9",
    "w_over_128_keys": "spatial_attn_kernel at 132 keys + temporal_fused (width), traj_fused (height)",
    "h_under_8_keys": "spatial_attn_kernel at 4 keys + temporal_fused (height), traj_fused (width)",
    "maps_temporal_fused": "spatial_attn_kernel writing both attention maps + temporal_fused",
    "t13_reassoc": "temporal_stream_kernel: online maximum over 13 frames, reassociated",
    "t13_no_reassoc": "temporal_attn_kernel: online maximum over 13 frames, k2 with its bias",
    "generic_c64": "generic tier, head dim 8, temporal_attn_kernel at T = 3",
    "full_272_keys": "spatial_attn_long_kernel, two key chunks (256 + 16)",
    "full_576_keys": "spatial_attn_long_kernel, three key chunks (256 + 256 + 64)",
    "cc_ln_in_kernel": "cross-clip flavour on traj_fused, the post-norm in the kernel",
    "cc_ln_own_launch": "cross-clip flavour on the generic tier (T = 13, reassociated), the post-norm in its own launch",
}
CHUNKED = ("full_272_keys", "full_576_keys")
CC_ATTN = "transformer_trajectory_self_attention_layers.0.self_attn"

# PAIRS_BEGIN (python tests/infer_regime_cases.py prints these lines)
PAIRS = {
    ("mq2_ffn_rides", "shift"): Pair(0, dict(mk=400, mt=1600)),
    ("mq2_ffn_rides", "sharp_s"): Pair(0, dict(gs=8)),
    ("mq2_ffn_rides", "sharp_t"): Pair(0, dict(gt=120)),
    ("mq1_frames_32_48", "shift"): Pair(0, dict(mk=400, mt=1600)),
    ("mq1_frames_32_48", "sharp_s"): Pair(1, dict(gs=8)),
    ("mq1_frames_32_48", "sharp_t"): Pair(7, dict(gt=80)),
    ("first_on_64_rows", "shift"): Pair(0, dict(mk=400, mt=1600)),
    ("first_on_64_rows", "sharp_s"): Pair(0, dict(gs=8)),
    ("first_on_64_rows", "sharp_t"): Pair(0, dict(gt=120)),
    ("rows16_merged", "shift"): Pair(0, dict(mk=400, mt=1600)),
    ("rows16_merged", "sharp_s"): Pair(1, dict(gs=8)),
    ("rows16_merged", "sharp_t"): Pair(0, dict(gt=80)),
    ("rows16_ragged", "shift"): Pair(0, dict(mk=400, mt=1600)),
    ("rows16_ragged", "sharp_s"): Pair(1, dict(gs=8)),
    ("rows16_ragged", "sharp_t"): Pair(0, dict(gt=120)),
    ("rows32_merged_split2", "shift"): Pair(0, dict(mk=400, mt=1600)),
    ("rows32_merged_split2", "sharp_s"): Pair(0, dict(gs=8)),
    ("rows32_merged_split2", "sharp_t"): Pair(1, dict(gt=80)),
    ("t9_rows16", "shift"): Pair(0, dict(mk=400, mt=1600)),
    ("t9_rows16", "sharp_s"): Pair(1, dict(gs=8)),
    ("t9_rows16", "sharp_t"): Pair(0, dict(gt=60)),
    ("w_over_128_keys", "shift"): Pair(0, dict(mk=400, mt=1600)),
    ("w_over_128_keys", "sharp_s"): Pair(1, dict(gs=8)),
    ("w_over_128_keys", "sharp_t"): Pair(6, dict(gt=80)),
    ("h_under_8_keys", "shift"): Pair(0, dict(mk=400, mt=1600)),
    ("h_under_8_keys", "sharp_s"): Pair(1, dict(gs=12)),
    ("h_under_8_keys", "sharp_t"): Pair(0, dict(gt=60)),
    ("maps_temporal_fused", "shift"): Pair(0, dict(mk=400, mt=1600)),
    ("maps_temporal_fused", "sharp_s"): Pair(5, dict(gs=8)),
    ("maps_temporal_fused", "sharp_t"): Pair(5, dict(gt=80)),
    ("t13_reassoc", "shift"): Pair(0, dict(mk=400, mt=800)),
    ("t13_reassoc", "sharp_s"): Pair(0, dict(gs=12)),
    ("t13_reassoc", "sharp_t"): Pair(9, dict(gt=40)),
    ("t13_no_reassoc", "shift"): Pair(0, dict(mk=400, mt=800)),
    ("t13_no_reassoc", "sharp_s"): Pair(0, dict(gs=12)),
    ("t13_no_reassoc", "sharp_t"): Pair(9, dict(gt=40)),
    ("generic_c64", "shift"): Pair(0, dict(mk=800, mt=800)),
    ("generic_c64", "sharp_s"): Pair(0, dict(gs=8)),
    ("generic_c64", "sharp_t"): Pair(1, dict(gt=40)),
    ("full_272_keys", "shift"): Pair(0, dict(mk=400, mt=3200)),
    ("full_272_keys", "sharp_s"): Pair(4, dict(gs=32)),
    ("full_272_keys", "sharp_t"): Pair(1, dict(gt=320)),
    ("full_576_keys", "shift"): Pair(0, dict(mk=400, mt=3200)),
    ("full_576_keys", "sharp_s"): Pair(0, dict(gs=32)),
    ("full_576_keys", "sharp_t"): Pair(9, dict(gt=160)),
    ("cc_ln_in_kernel", "shift"): Pair(0, dict(mk=800, mt=6400)),
    ("cc_ln_in_kernel", "sharp_s"): Pair(0, dict(gs=48)),
    ("cc_ln_own_launch", "shift"): Pair(0, dict(mk=800, mt=3200)),
    ("cc_ln_own_launch", "sharp_s"): Pair(1, dict(gs=32)),
    ("cc_ln_own_launch", "sharp_t"): Pair(0, dict(gt=480)),
}
# pairs that cannot meet the logit conditions, the coverage and YARD_CAP at once (at most 3, no case entirely)
LEFT_OUT = {
    ("cc_ln_in_kernel", "sharp_t"): "logit condition: the widest temporal range stays under 120 on all 16 seeds at the ladder's last rung "
                                    "(gt = 480: 78 .. 119.9); the layer-normed clip queries give temporal logits of 0.2 as drawn",
}
# PAIRS_END


def pair_ids():
    return [(n, r) for n in CASES for r in REGIMES if (n, r) not in LEFT_OUT]


def case(name):
    return ipc.CASES[name]


def passes(name):
    """[(figure key, parameter prefix, stage-name prefix, keys per frame)]"""
    c = case(name)
    if c.kind == "axial":
        return [("h", "height_attn", "h.", c.H), ("w", "width_attn", "w.", c.W)]
    if c.kind == "full":
        return [("t", "temporal_attn", "", c.H * c.W)]
    return [("cc", CC_ATTN, "", c.H)]


def forms(name):
    """[(Q, temporal form)] per pass, from the stage names recorded for the case"""
    c = case(name)
    reassoc = c.C == 256 and c.T >= 12 and not any(k == "generic_only" or (k == "plan_force" and v & 64) for k, v in c.options)
    return [fs.sites(ipc.STAGES[name], sp, reassoc) for _, _, sp, _ in passes(name)]


def regime_weights(name, offset, regime, mult):
    """ipc._weights at seed SEED + offset with the regime's multipliers applied in fp32: the device, the oracle and the yardstick get the
    same parameters"""
    c = case(name)
    w = dict(ipc._weights(c, ipc.SEED + offset))
    if regime is None:
        return w
    C = c.C

    def scaled(key, m, rows=None):
        t = w[key].clone()
        if rows is None:
            t *= float(m)
        else:
            t[rows] *= float(m)
        w[key] = t

    for _, prefix, _, _ in passes(name):
        fused_qkv = c.kind == "cc"
        if regime == "shift":
            scaled(f"{prefix}.qkv.bias", mult["mk"], slice(C, 2 * C)) if fused_qkv else scaled(f"{prefix}.k.bias", mult["mk"])
            scaled(f"{prefix}.proj_kv.bias", mult["mt"], slice(0, C))
        elif regime == "sharp_s":
            for k in ("weight", "bias"):
                scaled(f"{prefix}.qkv.{k}", mult["gs"], slice(0, C)) if fused_qkv else scaled(f"{prefix}.q.{k}", mult["gs"])
        elif regime == "sharp_t":
            for k in ("weight", "bias"):
                scaled(f"{prefix}.proj_q.{k}", mult["gt"])
        else:
            raise KeyError(regime)
    return w


# ---- the oracle's two softmaxes, watched ----------------------------------------------------------------------------------------------
@contextlib.contextmanager
def watched(watch):
    """Around a float64 run of the oracle: `watch` receives one dict of figures per pass.  _trajectory_core takes the spatial softmax over
    dim -1 of [S, h, N, L] logits once per frame and the temporal one over dim 2 of [S, N, T, h] once per pass; any other softmax (the
    cross-clip class head's) passes through."""
    spatial = []

    def softmax(x, dim):
        if dim == -1 and x.dim() == 4:
            spatial.append(_spatial_figures(x.detach().double()))
        elif dim == 2 and x.dim() == 4:
            fig = dict(maxabs=max(f["maxabs"] for f in spatial), range=max(f["range"] for f in spatial),
                       last_tile=any(f["last_tile"] for f in spatial), key0=any(f["key0"] for f in spatial),
                       chunks=sorted(set().union(*(f["chunks"] for f in spatial))), jump=any(f["jump"] for f in spatial))
            watch.append(dict(spatial=fig, temporal=_temporal_figures(x.detach().double())))
            spatial.clear()
        return torch.softmax(x, dim=dim)

    real = orc.torch
    orc.torch = trc._Torch(softmax)
    try:
        yield
    finally:
        orc.torch = real


class _TorchExpAsP:
    """the torch module as the WRONG softmaxes see it, with exp rounded to fp16 the way the kernels round exp2(s - m) into the P operand:
    what overflows fp16 (s - m above 11.09) becomes inf there"""

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def exp(x):
        return fs.f16(torch.exp(x))


def wrong_softmax(name, wrong):
    """fs.Softmax of WRONG[wrong].  The spatial one rounds its exponentials as the P operand itself (f16_sites.core does not round a
    replaced softmax's probabilities again); the temporal one stays in the run's dtype, as the kernels' is in fp32.  The inference kernels
    are instantiated per frame count or stream over the frames, so none has a dead slot by design: dead_slots_as_zero counts ONE, what an
    instantiation for T + 1 frames would."""
    sp, tp = WRONG[wrong][0], WRONG[wrong][1]
    T = case(name).T

    def spatial(lg):
        real = trc.torch
        trc.torch = _TorchExpAsP()
        try:
            return sp(lg)
        finally:
            trc.torch = real

    return fs.Softmax(spatial if sp else None, (lambda t: tp(t, T + 1)) if tp else None)


# ---- one forward: float64 oracle, yardstick ---------------------------------------------------------------------------------------------
_runs = {}


def _key(name, offset, regime, mult):
    return (name, offset, regime, tuple(sorted((mult or {}).items())))


def _ins(name, dtype):
    return [x.to(dtype) for x in ipc._inputs(case(name))]


def oracle(name, offset, regime, mult):
    """float64 oracle of the case at weight seed SEED + offset under `regime` (None: as drawn) -> {label: tensor} in the labels of ipc.run,
    with the softmaxes' figures per pass under "figures".  Computed once per argument set and shared: leave it unchanged."""
    key = _key(name, offset, regime, mult) + ("oracle",)
    if key not in _runs:
        c = case(name)
        w = {k: v.double() for k, v in regime_weights(name, offset, regime, mult).items()}
        ins, watch = _ins(name, torch.float64), []
        with watched(watch):
            if c.kind == "cc":
                r = orc.cross_clip_module(ins[0], ins[1], w, ipc.CC_LAYERS, ipc.CC_PIXELS[0])
                res = dict(out=r["pred_masks"], pred_logits=r["pred_logits"])
            elif c.kind == "full":
                res = dict(out=orc.trajectory_layer(ins[0], ins[1], w, HEADS))
            else:
                want = bool(c.extras.get("return_attn"))
                out, ha, wa = orc.axial_layer(ins[0], ins[1], w, HEADS, want_attn=want)
                res = dict(out=out, h_attn=ha, w_attn=wa) if want else dict(out=out)
        res["figures"] = watch
        _runs[key] = res
    return _runs[key]


def emulate(name, offset, regime, mult, wrong=None, dtype=torch.float64):
    """the yardstick (f16_sites in `dtype` with the sites of the case's kernel forms) on the same inputs and weights -> {label: tensor};
    wrong: a key of WRONG, that softmax in place of the right one (not kept)"""
    key = _key(name, offset, regime, mult) + ("emulation", dtype)
    if wrong is None and key in _runs:
        return _runs[key]
    c = case(name)
    w = {k: v.to(dtype) for k, v in regime_weights(name, offset, regime, mult).items()}
    ins = _ins(name, dtype)
    qf = forms(name)
    sm = wrong_softmax(name, wrong) if wrong else None
    if c.kind == "cc":
        q, form = qf[0]
        real = orc.cc_trajectory_attention
        orc.cc_trajectory_attention = lambda x, wl, seq_len, num_frames, heads=HEADS, attn_keep=None: fs.cc_traj(x, wl, num_frames, heads, q, form, sm)
        try:
            r = orc.cross_clip_module(ins[0], ins[1], w, ipc.CC_LAYERS, ipc.CC_PIXELS[0])
        finally:
            orc.cc_trajectory_attention = real
        res = dict(out=r["pred_masks"], pred_logits=r["pred_logits"])
    elif c.kind == "full":
        res = dict(out=fs.full_layer(ins[0], ins[1], w, HEADS, qf[0][0], qf[0][1], sm))
    else:
        maps = [] if c.extras.get("return_attn") else None
        out = fs.layer(ins[0], ins[1], w, HEADS, (qf[0][0], qf[1][0]), (qf[0][1], qf[1][1]), sm, maps)
        res = dict(out=out, h_attn=maps[0], w_attn=maps[1]) if maps else dict(out=out)
    if wrong is None:
        _runs[key] = res
    return res


def is_map(label):
    return label.endswith("_attn")


def err(label, got, ref):
    """an output tensor: the worse of max|a - b| / max|b| and relative L2; a map: max |dp|"""
    if is_map(label):
        return float((got.double() - ref.double()).abs().max())
    return max(rel_err(got, ref), rel_l2(got, ref))


def labels(res):
    return [k for k in res if k != "figures"]


def yard_errors(name, offset, regime, mult):
    ref, emu = oracle(name, offset, regime, mult), emulate(name, offset, regime, mult)
    return {k: err(k, emu[k], ref[k]) for k in labels(emu)}


_yards = {}


def yardstick(name, regime):
    """y per output label of the stored pair: the emulation's largest distance from float64 over YARD_SEEDS weight seeds (the pair's own
    first), at the pair's multipliers.  CPU; computed once."""
    if (name, regime) not in _yards:
        pair = PAIRS[name, regime]
        ys = [yard_errors(name, pair.offset + i, regime, pair.mult) for i in range(YARD_SEEDS)]
        _yards[name, regime] = {k: max(y[k] for y in ys) for k in ys[0]}
        for i in range(1, YARD_SEEDS):                  # the other seeds' runs are needed by nothing else
            for kind in (("oracle",), ("emulation", torch.float64)):
                _runs.pop(_key(name, pair.offset + i, regime, pair.mult) + kind, None)
    return _yards[name, regime]


def reference(name, regime):
    pair = PAIRS[name, regime]
    return oracle(name, pair.offset, regime, pair.mult)


def plain(name, regime):
    return oracle(name, PAIRS[name, regime].offset, None, None)


def pair_weights(name, regime, plain_weights=False):
    pair = PAIRS[name, regime]
    return regime_weights(name, pair.offset, None if plain_weights else regime, pair.mult)


# ---- the screening conditions -----------------------------------------------------------------------------------------------------------
def logit_misses(name, regime, figures):
    out = []
    for (key, *_), fig in zip(passes(name), figures):
        for half in ("spatial", "temporal"):
            lo_abs, lo_range, hi_range = LOGIT[regime][half]
            f = fig[half]
            if lo_abs is not None and not f["maxabs"] >= lo_abs:
                out.append(f"{key}.{half}: largest |s| {f['maxabs']:.4g} < {lo_abs}")
            if lo_range is not None and not f["range"] >= lo_range:
                out.append(f"{key}.{half}: widest range {f['range']:.4g} < {lo_range}")
            if hi_range is not None and not f["range"] < hi_range:
                out.append(f"{key}.{half}: widest range {f['range']:.4g} >= {hi_range}")
    return out


def coverage_misses(name, regime, figures):
    """the training file's coverage, for this tier: 16-key tiles (a 32-key step is two of them), 256-key chunks of the long kernel"""
    out, T = [], case(name).T
    for (key, _, _, L), fig in zip(passes(name), figures):
        sp, tp = fig["spatial"], fig["temporal"]
        if regime == "sharp_s":
            if not sp["last_tile"]:
                out.append(f"{key}: no arg-max key in the last key tile with weight above 0.99")
            if not sp["key0"]:
                out.append(f"{key}: no arg-max at key 0")
            if name in CHUNKED:
                if sp["chunks"] != list(range(-(-L // trc.K_CHUNK))):
                    out.append(f"{key}: arg-max keys in chunks {sp['chunks']} only")
                if not sp["jump"]:
                    out.append(f"{key}: no arg-max in the last key chunk more than {EXP_UNDERFLOW} above the earlier chunks")
        if regime == "sharp_t" and tp["frames"] != list(range(T)):
            out.append(f"{key}: frames {tp['frames']} of {T} take a weight above 0.99")
    return out


def screen(name, regime, offset, mult, logit_only=False):
    """-> (misses, report): the screening conditions of (case, regime) at this weight-seed offset and these multipliers"""
    ref = oracle(name, offset, regime, mult)
    report = dict(figures=ref["figures"])
    misses = logit_misses(name, regime, ref["figures"])
    if logit_only:
        return misses, report
    misses += coverage_misses(name, regime, ref["figures"])
    if misses:
        return misses, report
    if not all(bool(torch.isfinite(ref[k]).all()) for k in labels(ref)):
        return ["the oracle is not finite"], report
    report["yard"] = y = yard_errors(name, offset, regime, mult)
    worst = max((k for k in y if not is_map(k)), key=y.get)
    if not y[worst] <= YARD_CAP:
        misses.append(f"yardstick {worst} {y[worst]:.3e} > {YARD_CAP}")
    return misses, report


def tag(name, regime):
    """the pair, its multipliers and seed offset, and the float64 logits' largest |s| and widest range per pass and half"""
    pair = PAIRS[name, regime]
    figs = "; ".join(f"{key}: spatial |s| {f['spatial']['maxabs']:.4g} range {f['spatial']['range']:.4g}, temporal |s| {f['temporal']['maxabs']:.4g} "
                     f"range {f['temporal']['range']:.4g}" for (key, *_), f in zip(passes(name), reference(name, regime)["figures"]))
    return f"{name} {regime} {' '.join(f'{k}={v}' for k, v in pair.mult.items())} seed+{pair.offset} [{figs}]"


def describe(report):
    lines = []
    for i, fig in enumerate(report["figures"]):
        sp, tp = fig["spatial"], fig["temporal"]
        lines.append(f"pass {i}: spatial |s| <= {sp['maxabs']:.4g}, range <= {sp['range']:.4g}; temporal |s| <= {tp['maxabs']:.4g}, "
                     f"range <= {tp['range']:.4g}, one-hot frames {tp['frames']}")
    if "yard" in report:
        lines.append("yardstick vs float64: " + ", ".join(f"{k} {v:.3e}" for k, v in report["yard"].items()))
    return lines


# ---- the bounds -------------------------------------------------------------------------------------------------------------------------
def missed(name, regime, got, log=None, tag=""):
    """The bounds on one forward `got` ({label: tensor} of ipc.run, on the CPU) of the stored pair -> the list of those it misses."""
    ref, y = reference(name, regime), yardstick(name, regime)
    bad = [k for k in labels(ref) if not bool(torch.isfinite(got[k]).all())]
    if bad:
        return [f"not finite: {bad}"]
    out = []
    for k in labels(ref):
        e = err(k, got[k], ref[k])
        bound = max(TOL_MAP if is_map(k) else TOL_F16, YARD_FACTOR * y[k])
        if log is not None:
            log.append(f"{tag} {k} error={e:.3e} yardstick={y[k]:.3e} ratio={e / y[k]:.3g} bound={bound:.3e}")
        if not e <= bound:
            out.append(f"{k}: error {e:.3e} > {bound:.3e} (yardstick {y[k]:.3e})")
        if is_map(k):
            rows = float((got[k].double().sum(-1) - 1).abs().max())
            if not rows <= 1e-5:
                out.append(f"{k}: rows sum to 1 within {rows:.3e} > 1e-5")
    return out


def plain_missed(name, regime, got):
    """the standing 1e-3 bar on the pair's seed with the weights as drawn"""
    ref = plain(name, regime)
    e, e2 = rel_err(got["out"], ref["out"]), rel_l2(got["out"], ref["out"])
    return [] if e < TOL_F16 and e2 < TOL_F16 else [f"plain weights: max/max {e:.3e} relL2 {e2:.3e} >= {TOL_F16}"]


# ---- the search that filled PAIRS -------------------------------------------------------------------------------------------------------
def rung_below(regime, mult):
    """the multipliers one ladder rung lower, one dict per multiplier that has a lower rung"""
    out = []
    for k, v in mult.items():
        i = LADDER[regime].index(v)
        if i > 0:
            out.append({**mult, k: LADDER[regime][i - 1]})
    return out


def _shift_rungs(name, offset):
    """the first rungs of mk and of mt at which every pass's largest |s| reaches the condition at this seed (the two are independent:
    k.bias moves the spatial logits only, proj_kv.bias the temporal ones only)"""
    found = {}
    for rung in LADDER["shift"]:
        fig = oracle(name, offset, "shift", dict(mk=rung, mt=rung))["figures"]
        for which, k in (("spatial", "mk"), ("temporal", "mt")):
            if k not in found and all(f[which]["maxabs"] >= LOGIT["shift"][which][0] for f in fig):
                found[k] = rung
        if len(found) == 2:
            return found
    return None


def search(name, regime):
    """the first ladder rung and the first of SEEDS offsets at which `screen` holds (shift: per offset, the first rung of each half)"""
    why = {}
    if regime == "shift":
        for offset in range(SEEDS):
            mult = _shift_rungs(name, offset)
            misses, report = screen(name, regime, offset, mult) if mult else (["no rung of the ladder meets the logit conditions"], None)
            if not misses:
                return Pair(offset, mult), report, why
            why[offset] = [f"{mult}"] + misses
            _runs.clear()
        return None, None, why
    k = {"sharp_s": "gs", "sharp_t": "gt"}[regime]
    for rung in LADDER[regime]:
        for offset in range(SEEDS):
            misses, report = screen(name, regime, offset, {k: rung})
            if not misses:
                return Pair(offset, {k: rung}), report, why
            why[rung, offset] = misses
        _runs.clear()
    return None, None, why


if __name__ == "__main__":
    for name in CASES:
        for regime in REGIMES:
            if len(sys.argv) > 1 and name not in sys.argv[1:] and regime not in sys.argv[1:]:
                continue
            pair, report, why = search(name, regime)
            _runs.clear()
            if pair is None:
                print(f'    # ("{name}", "{regime}"): no seed; ' + "; ".join(f"{o}: {m}" for o, m in list(why.items())[-3:]), flush=True)
                continue
            print(f'    ("{name}", "{regime}"): {pair},', flush=True)
            for line in describe(report):
                print("    #   " + line, flush=True)
