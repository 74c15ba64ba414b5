"""Cases for the three eval-forward attention kernels off the regime their own case files draw from (N(0, 1) inputs, soft softmax, attention
masks from the signs of random logits):

  A  m2f_attn_kernel / m2f_attn_combine_kernel under attention masks built by hand -- one open key, one live key chunk, a masked 16-key step
     at the head of a live chunk, open keys only in the last 32-bit word -- at case e of m2f_decoder_cases (24, 70 and 598 keys: one, one and
     three chunks) and at the key-chunk cap (16928 keys: 59 chunks of 288);
  B  m2f_logits_kernel on mask features solved for, so that the float64 logits of a layer are +-1 in a chosen pattern: rows with one open
     key, all-masked and all-open rows, and no logit anywhere near the rounding band;
  C  all three kernels with the scores scaled by g in (0, 1, 8, SHARP): uniform weights at 0, almost one-hot weights at SHARP, where the
     largest score is past fp32 exp's overflow and the score range past its underflow.

The yardstick is the float64 restatement of the kernels' own case modules; the bound is 8 x the float32 restatement's own max-norm error on
the same inputs, per compared tensor, and 8 * 2^-24 * max|float64 output| where that error is below one rounding of the output (`bound`).
`wrong=` states the attention wrongly on purpose in the ways a kernel of this kind can be (test_attention_edges_cpu.py checks that these
cases tell each of them from the right one).
"""
from collections import OrderedDict
import math

import torch
import torch.nn.functional as F

import kmax_decoder_cases as kc
import kmax_pixel_decoder_cases as pc
import m2f_decoder_cases as mc

FLOOR = 2.0 ** -24
# the factor of the sharpest class per kernel: the first of 64, 128, ... at which the float64 run meets the conditions of
# test_attention_edges_cpu.py::test_sharp_conditions (median largest weight > 0.9, a score > 89, a score range > 104)
SHARP = dict(m2f=64, kmax=64, kpix=64)
EXP_OVERFLOW, EXP_UNDERFLOW = 89.0, 104.0      # fp32: exp(x) = inf past 88.73; exp(-x) = 0 past 103.98


def classes(kernel):
    return (0, 1, 8, SHARP[kernel])


def err(a, b):
    return float((a.double().cpu() - b.double().cpu()).abs().max())


def bound(own, want):
    """(bound, the float32 restatement's error, floor used) of one compared tensor"""
    e, top = err(own, want), float(want.abs().max())
    if e < FLOOR * top:
        return 8 * FLOOR * top, e, True
    return 8 * e, e, False


def row_stats(scores, weights):
    """per softmax row: the largest weight, the largest score, the range of the scores of its open keys (-inf = masked), the largest
    departure of an open key's weight from 1 / (open keys)"""
    is_open = scores != -math.inf
    n_open = is_open.sum(-1, keepdim=True).clamp(min=1).to(weights.dtype)
    smax = scores.max(-1)[0]
    smin = scores.masked_fill(~is_open, math.inf).min(-1)[0]
    uni = ((weights - 1.0 / n_open).abs() * is_open).max(-1)[0]
    return dict(top=weights.max(-1)[0].flatten(), smax=smax.flatten(), srange=(smax - smin).flatten(), uniform=uni.flatten())


# ==== A. hand-built attention masks =====================================================================================================
KEY_CHUNK, MAX_CHUNKS = 256, 64          # kM2fKeyChunk, kM2fMaxChunks (axvs_m2f.h)


def chunks_of(S):
    return min((S + KEY_CHUNK - 1) // KEY_CHUNK, MAX_CHUNKS)


def chunk_of(S):
    """chunk_of() of axvs_m2f.hip: keys per attention workgroup"""
    n = chunks_of(S)
    return ((S + n - 1) // n + 31) // 32 * 32


def _rows(open_patterns, Q, N):
    """open patterns [n][S] -> masked [N, Q, S]: row q takes pattern q mod n, so every 16-query tile meets every pattern"""
    P = torch.stack(open_patterns)
    return ~P[torch.arange(Q) % len(open_patterns)].unsqueeze(0).repeat(N, 1, 1)


def one_open_positions(S, chunk):
    out = []
    for p in (0, 15, 16, 31, 32, chunk - 1, chunk, 2 * chunk - 1, S - 2, S - 1):
        if 0 <= p < S and p not in out:
            out.append(p)
    return out


def one_open(S, chunk, Q, N=1, positions=None):
    k = torch.arange(S)
    return _rows([k == p for p in (one_open_positions(S, chunk) if positions is None else positions)], Q, N)


def one_chunk(S, chunk, Q, N=1, chunks=None):
    k, n = torch.arange(S), (S + chunk - 1) // chunk
    pats = [(k >= c * chunk) & (k < (c + 1) * chunk) for c in (range(n) if chunks is None else chunks)]
    pats.append(k == S - 1)          # of the last chunk, only its last key
    return _rows(pats, Q, N)


def hand_masks(S, chunk, Q, N=1):
    """name -> bool [N, Q, S], True = key masked"""
    k = torch.arange(S)
    r, step = k % chunk, k // 16
    tail = 32 * (S // 32) if S % 32 else S - 32
    return OrderedDict(
        one_open=one_open(S, chunk, Q, N),
        one_chunk=one_chunk(S, chunk, Q, N),
        head_step_masked=_rows([(r >= 16) & (k % 2 == 0), (r >= 16) & (k % 2 == 1)], Q, N),
        tail_word=_rows([k >= tail], Q, N),
        alternate=_rows([k % 2 == 0, k % 2 == 1, step % 2 == 0, step % 2 == 1], Q, N),
        all_open=torch.zeros(N, Q, S, dtype=torch.bool),
        all_masked=torch.ones(N, Q, S, dtype=torch.bool))


class M2fEdge(mc.Restatement):
    """mc.Restatement with nn.MultiheadAttention written out (test_attention_edges_cpu.py: equal to it to 1e-12 in float64), so that the
    scores can be recorded (`stats[(layer, attention)]`) and the attention stated wrongly:
      no_max                 softmax as exp(s) / sum exp(s)
      chunk_local_max        (cross-attention) a softmax per key chunk, each under its own maximum, joined without e^(m_c - M)
      masked_chunk_uniform   (cross-attention) a wholly masked key chunk contributes uniform weights: its scores count as 0
      no_all_masked_rule     (cross-attention) a row whose keys are all masked attends to nothing"""

    def __init__(self, params, mask_features, memories, dtype, layers, wrong=None):
        super().__init__(params, mask_features, memories, dtype, layers)
        self.wrong, self.stats, self._dead = wrong, {}, None

    def layer(self, i, x, masked):
        self._dead = masked.all(-1)                                         # [N, Q], before the all-masked rule
        return super().layer(i, x, masked)

    def _attend(self, a, s, v):
        """scores [N*8, Q, S] (-inf = masked), values [N*8, S, 32] -> (weights or None, retrieved [N*8, Q, 32])"""
        cross = a == 0
        if self.wrong == "no_max":
            e = s.exp()
            w = e / e.sum(-1, keepdim=True)
        elif self.wrong == "chunk_local_max" and cross:
            S = s.shape[-1]
            chunk = chunk_of(S)
            num = den = 0.0
            for s0 in range(0, S, chunk):
                sc = s[..., s0:s0 + chunk]
                p = (sc - sc.max(-1, keepdim=True)[0]).exp()                # -inf - -inf = nan where the whole chunk is masked
                num, den = num + p @ v[:, s0:s0 + chunk], den + p.sum(-1, keepdim=True)
            return None, num / den
        elif self.wrong == "masked_chunk_uniform" and cross:
            S = s.shape[-1]
            chunk = chunk_of(S)
            s = s.clone()
            for s0 in range(0, S, chunk):
                sc = s[..., s0:s0 + chunk]
                sc[(sc == -math.inf).all(-1)] = 0.0
            w = F.softmax(s, dim=-1)
        else:
            w = F.softmax(s, dim=-1)
        if self.wrong == "no_all_masked_rule" and cross:
            w = w * (~self._dead).repeat_interleave(mc.HEADS, dim=0).unsqueeze(-1)
        return w, w @ v

    def _attn(self, i, a, query, key, value, query_pos, key_pos, mask):
        C, H = mc.C, mc.HEADS
        p = f"transformer_decoder.layers.{i}.attentions.{a}.attn."
        W, b = self.p[p + "in_proj_weight"], self.p[p + "in_proj_bias"]
        q = F.linear(query + query_pos, W[:C], b[:C])
        k = F.linear(key + key_pos, W[C:2 * C], b[C:2 * C])
        v = F.linear(value, W[2 * C:], b[2 * C:])
        Lq, N, S = q.shape[0], q.shape[1], k.shape[0]
        heads = lambda t, n: t.reshape(n, N * H, C // H).transpose(0, 1)     # batch index n * 8 + h, nn.MultiheadAttention's
        s = (heads(q, Lq) / math.sqrt(C // H)) @ heads(k, S).transpose(1, 2)
        if mask is not None:
            s = s.masked_fill(mask, -math.inf)
        w, o = self._attend(a, s, heads(v, S))
        if w is not None:
            self.stats[(i, a)] = row_stats(s, w)
        o = o.transpose(0, 1).reshape(Lq, N, C)
        return query + F.linear(o, self.p[p + "out_proj.weight"], self.p[p + "out_proj.bias"])


CAP = mc.Case("cap", 707, 1, 8, 2, (4, 4), ((92, 92), (2, 2), (2, 2)), 1, 3, 0.0)      # 16928 keys > 64 x 256: 59 chunks of 288
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        with torch.no_grad():
            _CACHE[key] = make()
    return _CACHE[key]


def _m2f_items(r64, r32, i, x_in, masks):
    """name -> dict(masked, want [Q,N,C], tol, own, floor) of layer i on queries x_in [Q,N,C] (float64) under each mask"""
    out = OrderedDict()
    for name, m in masks.items():
        want = r64.layer(i, x_in, m)
        tol, own, floor = bound(r32.layer(i, x_in.float(), m), want)
        out[name] = dict(masked=m, want=want, tol=tol, own=own, floor=floor)
    return out


def m2f_mask_study(layer):
    """layer 0..2 of case e (Q = 100: the last query tile has 4 rows) under the hand-built masks, on the float64 chain's queries"""
    def make():
        st = mc.study(mc.BY_NAME["e"])
        case, S = st["case"], mc.keys_of(st["case"], layer % 3)
        x_in = st["layers"][layer]["x_in"]
        return dict(st=st, S=S, chunk=chunk_of(S), x_in=x_in,
                    items=_m2f_items(st["r64"], st["r32"], layer, x_in, hand_masks(S, chunk_of(S), case.Q, case.N)))
    return _cached(("m2f_masks", layer), make)


def cap_inputs():
    def make():
        params, (mf, mems) = mc.make_params(CAP), mc.make_inputs(CAP)
        S = mc.keys_of(CAP, 0)
        chunk = chunk_of(S)
        n = (S + chunk - 1) // chunk
        g = torch.Generator().manual_seed(CAP.seed + 2)
        masks = OrderedDict(
            one_open=one_open(S, chunk, CAP.Q, 1, (0, 32, chunk - 1, chunk, 30 * chunk + 17, (n - 1) * chunk - 1, S - 2, S - 1)),
            one_chunk=one_chunk(S, chunk, CAP.Q, 1, (0, 30, n - 1)),
            half=torch.rand(1, CAP.Q, S, generator=g) < 0.5)
        return dict(params=params, mf=mf, mems=mems, S=S, chunk=chunk, nchunk=n, masks=masks)
    return _cached("cap_inputs", make)


def m2f_cap_study():
    def make():
        c = cap_inputs()
        r64 = mc.Restatement(c["params"], c["mf"], c["mems"], torch.float64, 1)
        r32 = mc.Restatement(c["params"], c["mf"], c["mems"], torch.float32, 1)
        x_in = r64.start()
        return dict(c, x_in=x_in, r64=r64, items=_m2f_items(r64, r32, 0, x_in, c["masks"]))
    return _cached("m2f_cap", make)


# ==== B. the mask head on sparse rows =====================================================================================================
def sparse_rows_study(level):
    """Mask features at the size of level `level` of case e (the resize is the identity), solved for so that the float64 mask logits of the
    chain's queries in front of layer `level` are +-1 in a pattern chosen per row: row q takes kind q mod n of `kinds`."""
    def make():
        st = mc.study(mc.BY_NAME["e"])
        case = st["case"]
        S, (hl, wl) = mc.keys_of(case, level), case.levels[level]
        x_in = st["layers"][level]["x_in"]
        _, me = st["r64"].mask_embed(x_in)                                   # [1, Q, C], rank Q < C
        k = torch.arange(S)
        tail = 32 * (S // 32) if S % 32 else S - 32
        kinds = OrderedDict((f"one_open_{p}", k == p) for p in dict.fromkeys((0, S - 1, tail, min(31, S - 2), min(32, S - 2))))
        g = torch.Generator().manual_seed(808 + level)
        kinds.update(all_masked=k < 0, all_open=k >= 0, alternate=k % 2 == 0, tail_word=k >= tail, half=torch.rand(S, generator=g) < 0.5)
        is_open = torch.stack(list(kinds.values()))[torch.arange(case.Q) % len(kinds)]           # [Q, S]
        target = torch.where(is_open, 1.0, -1.0).double()
        feat = (torch.linalg.pinv(me[0]) @ target).float()                   # [C, S]: me . feat = target up to the rounding to fp32
        mf = feat.view(mc.C, case.T, hl, wl).permute(1, 0, 2, 3)[None].contiguous()
        r64 = mc.Restatement(st["params"], mf, st["mems"], torch.float64, case.layers)
        r32 = mc.Restatement(st["params"], mf, st["mems"], torch.float32, case.layers)
        logits = r64.head_logits(x_in, level)
        band = 8 * err(r32.head_logits(x_in.float(), level), logits)
        return dict(st=st, S=S, level=level, x_in=x_in, mf=mf, kinds=list(kinds), is_open=is_open[None], logits=logits, masked=logits < 0, band=band)
    return _cached(("sparse_rows", level), make)


# ==== C. sharp and uniform softmax ==========================================================================================================
# ---- m2f: g on the q rows of one attention's in_proj, in every layer of the case
M2F_SHARP_CASES = ("c", "e")


def m2f_variants():
    """(g, attention): class 1 once, the others once for the cross-attention (0) and once for the self-attention (1)"""
    return [(1, 0)] + [(g, a) for g in classes("m2f") if g != 1 for a in (0, 1)]


def m2f_scaled_params(params, layers, g, a):
    out = OrderedDict((k, v.clone()) for k, v in params.items())
    for i in range(layers):
        p = f"transformer_decoder.layers.{i}.attentions.{a}.attn."
        out[p + "in_proj_weight"][:mc.C] *= g
        out[p + "in_proj_bias"][:mc.C] *= g
    return out


def m2f_sharp_study(name, g, a, wrong=None):
    """every layer of case `name` on the float64 chain's queries with float64's own bits, the scores of attention `a` times g.
    wrong=None: per layer dict(want, tol, own, floor) and the float64 scores' row_stats; else the wrong float32 restatement's outputs."""
    def make():
        st = mc.study(mc.BY_NAME[name])
        case = st["case"]
        params = m2f_scaled_params(st["params"], case.layers, g, a)
        if wrong:
            r = M2fEdge(params, st["mf"], st["mems"], torch.float32, case.layers, wrong)
            return [r.layer(i, l["x_in"].float(), l["masked"]) for i, l in enumerate(st["layers"])]
        r64 = mc.Restatement(params, st["mf"], st["mems"], torch.float64, case.layers)
        r32 = mc.Restatement(params, st["mf"], st["mems"], torch.float32, case.layers)
        rec = M2fEdge(params, st["mf"], st["mems"], torch.float64, case.layers)
        layers = []
        for i, l in enumerate(st["layers"]):
            want = r64.layer(i, l["x_in"], l["masked"])
            tol, own, floor = bound(r32.layer(i, l["x_in"].float(), l["masked"]), want)
            layers.append(dict(want=want, tol=tol, own=own, floor=floor, written_out=rec.layer(i, l["x_in"], l["masked"]), stats=rec.stats[(i, a)]))
        return dict(st=st, params=params, layers=layers)
    return _cached(("m2f_sharp", name, g, a, wrong), make)


# ---- kmax: g on the similarity norm's gain of layer 0; one more class moves its bias by +50
KMAX_SHARP_CASES = ("c", "e")
_KMAX_SIM = "_kmax_transformer_layers.0._query_self_attention._batch_norm_similarity."


def kmax_classes():
    return [f"g{g}" for g in classes("kmax")] + ["bias50"]


class KmaxEdge(kc.Restatement):
    def __init__(self, params, case, dtype, wrong=None):
        super().__init__(params, case, dtype)
        self.wrong, self.stats = wrong, None

    def softmax(self, sim):
        if self.wrong == "no_max":
            e = sim.exp()
            w = e / e.sum(-1, keepdim=True)
        else:
            w = F.softmax(sim, dim=-1)
        self.stats = row_stats(sim, w)
        return w


def kmax_sharp_study(name, cls, wrong=None):
    """layer 0 of case `name` on the start queries under the hand map p % L, the similarity norm changed by class `cls`"""
    def make():
        case = kc.BY_NAME[name]
        params, (x, _) = kc.make_params(case), kc.make_inputs(case)
        params = OrderedDict((k, v.clone()) for k, v in params.items())
        if cls == "bias50":
            params[_KMAX_SIM + "bias"] += 50.0
        else:
            params[_KMAX_SIM + "weight"] *= float(cls[1:])
        level = kc.layer_levels(case)[0]
        S = case.T * case.levels[level][0] * case.levels[level][1]
        spread = torch.arange(case.B * S, dtype=torch.int64).view(case.B, S) % case.L
        stacked = kc.stack(x[level], case.B)
        if wrong:
            r = KmaxEdge(params, case, torch.float32, wrong)
            return r.layer(0, stacked, r.start(), index=spread)[0]
        r64, r32 = KmaxEdge(params, case, torch.float64), kc.Restatement(params, case, torch.float32)
        q_in = r64.start()
        want = r64.layer(0, stacked.double(), q_in, index=spread)[0]
        tol, own, floor = bound(r32.layer(0, stacked, q_in.float(), index=spread)[0], want)
        return dict(case=case, params=params, x=x[level], q_in=q_in, index=spread, want=want, tol=tol, own=own, floor=floor, stats=r64.stats)
    return _cached(("kmax_sharp", name, cls, wrong), make)


# ---- kpix: g on the q channels of the float64 chain's qkv rows; class 0 is the similarity norm's gain at 0
KPIX_SHARP_CASES = [(17, 33, 128, 2), (3, 128, 256, 1), (72, 2, 512, 1)]      # L = 128: both lane halves of the softmax; DK 64 / DV 128
_KPIX_AXIS = ("_stages.0._blocks.0._attention._height_axis.", "_stages.0._blocks.0._attention._width_axis.")


class KpixEdge(pc.Restatement):
    def __init__(self, params, dtype, wrong=None):
        super().__init__(params, dtype)
        self.wrong, self.stats = wrong, None

    def softmax(self, sim):
        if self.wrong == "no_max":
            e = sim.exp()
            w = e / e.sum(-1, keepdim=True)
        else:
            w = F.softmax(sim, dim=-1)
        self.stats = row_stats(sim, w)
        return w


def kpix_attend(r, qkv, axis):
    """one axis pass (0: along h, 1: along w) of restatement r on channels-last qkv rows [N, h, w, 4b] -> [N, h, w, 2b]"""
    N = qkv.shape[0]
    seq = qkv.permute(0, 2, 3, 1) if axis == 0 else qkv.permute(0, 1, 3, 2)                      # [N, other, 4b, L]
    got = r.attend(seq.reshape(-1, seq.shape[2], seq.shape[3]), _KPIX_AXIS[axis])
    got = got.reshape(N, -1, got.shape[1], got.shape[2])
    return got.permute(0, 3, 1, 2) if axis == 0 else got.permute(0, 1, 3, 2)


def kpix_params(spec, variant=None):
    """the stage case's parameters; variant "gain0": the similarity norms' gains 0; "offsets": their biases + 3, running means x 50"""
    params = OrderedDict((k, v.clone()) for k, v in pc.stage_study("axial", spec)["params"].items())
    for a in _KPIX_AXIS:
        if variant == "gain0":
            params[a + "_batch_norm_similarity.weight"] *= 0.0
        elif variant == "offsets":
            params[a + "_batch_norm_similarity.bias"] += 3.0
            params[a + "_batch_norm_similarity.running_mean"] *= 50.0
    return params


def kpix_sharp_study(spec, g, axis, wrong=None):
    def make():
        st = pc.stage_study("axial", spec)
        b = spec[2]
        qkv = st["rec"]["qkv_" + "hw"[axis]].clone()                        # [N, h, w, 4b] float64
        if g:
            qkv[..., :b] *= g
        params = kpix_params(spec, None if g else "gain0")
        if wrong:
            return kpix_attend(KpixEdge(params, torch.float32, wrong), qkv.float(), axis)
        r64 = KpixEdge(params, torch.float64)
        want = kpix_attend(r64, qkv, axis)
        tol, own, floor = bound(kpix_attend(pc.Restatement(params, torch.float32), qkv.float(), axis), want)
        return dict(case=st["case"], params=params, qkv=qkv, want=want, tol=tol, own=own, floor=floor, stats=r64.stats)
    return _cached(("kpix_sharp", spec, g, axis, wrong), make)
