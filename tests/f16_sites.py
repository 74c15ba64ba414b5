"""The 16-bit rounding sites of the inference tier, stated once: a torch-CPU restatement of the trajectory attention layers that rounds a
value to fp16 wherever the HIP pipeline does (MFMA operands, 16-bit intermediates in LDS / HBM) and nowhere else.  tools/error_budget.py
prices the sites with it; tests/infer_regime_cases.py runs it in float64 as the yardstick of the inference kernels off the soft-softmax
regime, where an fp16 logit of magnitude s carries an error of s * 2^-11 and no fixed tolerance holds.

Dtype-generic: every tensor takes the dtype of the inputs; `f16` rounds to fp16 and comes back to it.

A `Q` names the sites that round.  SITES are the 16 of the fused kernels.  One more switch is no site of its own:
  "psum"   the spatial denominator is the sum of the ROUNDED P (traj_fused's spatial half: ones . P^T on the matrix pipe, axvs_fused.h);
           off: the sum of the fp32 exponentials (spatial_attn_kernel and the fp32 `srun` of spatial_attn_long_kernel, axvs_attn.h).
`sites(stage_names)` gives the Q and the temporal form of a pass from the stage names the library reports for it.

`form` places the temporal half's sites where each kernel form rounds (axvs_api.hip, run_traj):
  "fused"    temporal_fused_kernel: q2 rounded as the operand of u = Wk2^T q2, u rounded as the operand of the logit MFMA, the K half of
             proj_kv.bias dropped (it cancels in the softmax over frames), sum_f a_f x_f accumulated in packed f16.
  "generic"  proj_q / proj_kv GEMMs into fp32 q2 and kv2 (k2 and v2 WITH their bias; operands x and the weights in 16 bits, the results are
             NOT rounded), temporal_attn_kernel in fp32; only o is rounded, as the operand of proj.
  "reassoc"  T >= 12: q2 (fp32 in HBM) rounded as the operand of the per-head GEMM u = Wk2^T q2, u kept in fp32, temporal_stream_kernel in
             fp32 on the 16-bit x, z = sum_f a_f x_f rounded ONCE as the operand of the per-head GEMM with Wv2.

`softmax`: None, or a Softmax(spatial, temporal) of functions logits -> probabilities in place of the right ones (either may be None);
a replaced spatial softmax hands its probabilities to the P operand as they are: it rounds its exponentials itself
(infer_regime_cases.wrong_softmax)."""
from collections import namedtuple

import torch

import axvs_oracle as orc

SITES = ["w_qkv", "w_temporal", "w_ffn", "a_qk", "a_v", "q", "k", "v", "p", "x", "q2", "qk", "xbar", "o", "y", "h"]
FORMS = ("fused", "generic", "reassoc")
Softmax = namedtuple("Softmax", "spatial temporal")


def f16(x):
    return x.to(torch.float16).to(x.dtype)


class Q:
    def __init__(self, on):
        self.on = set(on)

    def __call__(self, site, x):
        return f16(x) if site in self.on else x


def lin(x, w, name, q, wsite, bias=True):
    y = x @ q(wsite, w[name + ".weight"]).t()
    return y + w[name + ".bias"] if bias else y


def sites(stage_names, prefix="", reassoc=False):
    """(Q, form) of the pass whose stages carry `prefix` ("h.", "w." or "") among the library's stage names; reassoc: the planner
    reassociates the generic tier's temporal half (T >= 12 at C = 256 with 8 heads, unless plan_force 64 forbids it)"""
    mine = [n[len(prefix):] for n in stage_names if n.startswith(prefix)]
    traj_kernel = any(n.startswith(("traj_fused", "qkv+traj")) for n in mine)
    if traj_kernel or "temporal_fused" in mine:
        return Q(SITES + ["psum"] if traj_kernel else SITES), "fused"
    assert "temporal_attn" in mine, stage_names
    return Q(SITES), "reassoc" if reassoc else "generic"


def core(Qm, K, V, w, T, heads, q, form="fused", softmax=None, want_attn=False):
    """both halves on projected q (scaled, rounded), k, v [S, N, C] -> (out of proj, spatial maps [S h, N, T, L] or None)"""
    S, N, C = Qm.shape
    L, d = N // T, C // heads
    scale = d ** -0.5
    sp = lambda t: t.reshape(S, N, heads, d).permute(0, 2, 1, 3)
    Qh, Kh, Vh = sp(Qm), sp(K), sp(V)
    x = torch.empty(S, N, T, C, dtype=Qm.dtype)
    maps = torch.empty(S, heads, N, T, L, dtype=Qm.dtype) if want_attn else None
    for f in range(T):
        lg = Qh @ Kh[:, :, f * L:(f + 1) * L].transpose(-1, -2)
        if softmax is not None and softmax.spatial is not None:
            p = softmax.spatial(lg)
            xf = p @ Vh[:, :, f * L:(f + 1) * L]
        else:
            e = torch.exp(lg - lg.max(-1, keepdim=True).values)
            den = (q("p", e) if "psum" in q.on else e).sum(-1, keepdim=True)
            xf = (q("p", e) @ Vh[:, :, f * L:(f + 1) * L]) / den
            p = e / den                                                        # the maps are written from the fp32 exponentials
        if want_attn:
            maps[:, :, :, f] = p
        x[:, :, f] = xf.permute(0, 2, 1, 3).reshape(S, N, C)
    x = q("x", x)
    own = torch.arange(N) // L
    xd = x[:, torch.arange(N), own]
    q2 = lin(xd, w, "proj_q", q, "w_temporal") * scale
    Wkv = q("w_temporal", w["proj_kv.weight"])
    Wk2, Wv2 = Wkv[:C].reshape(heads, d, C), Wkv[C:]
    tsm = softmax.temporal if softmax is not None and softmax.temporal is not None else (lambda t: torch.softmax(t, 2))
    if form == "generic":
        kv2 = x @ Wkv.t() + w["proj_kv.bias"]                                   # [S,N,T,2C], fp32 in HBM
        tl = (q2.reshape(S, N, 1, heads, d) * kv2[..., :C].reshape(S, N, T, heads, d)).sum(-1)
        ta = tsm(tl)                                                            # [S,N,T,heads]
        o = (ta.unsqueeze(-1) * kv2[..., C:].reshape(S, N, T, heads, d)).sum(2).reshape(S, N, C)
    else:
        q2 = q("q2", q2).reshape(S, N, heads, d)
        qk = torch.einsum("snhd,hdc->snhc", q2, Wk2)                            # (Wk2_h^T q2_h): the k2 bias drops out of the softmax
        if form == "fused":
            qk = q("qk", qk)
        tl = torch.einsum("snhc,sntc->snth", qk, x)
        ta = tsm(tl)
        if form == "fused":
            xbar = torch.zeros(S, N, heads, C, dtype=Qm.dtype)
            for f in range(T):                                                  # packed-f16 running sum (v_pk_fma_f16)
                xbar = q("xbar", xbar + q("xbar", ta[:, :, f]).unsqueeze(-1) * x[:, :, f].unsqueeze(2))
        else:
            assert form == "reassoc", form
            xbar = q("xbar", torch.einsum("snth,sntc->snhc", ta, x))
        o = torch.einsum("snhc,hdc->snhd", xbar, Wv2.reshape(heads, d, C)).reshape(S, N, C) + w["proj_kv.bias"][C:]
    out = lin(q("o", o), w, "proj", q, "w_temporal")
    return out, (maps.reshape(S * heads, N, T, L) if want_attn else None)


def traj(kq, val, w, T, heads, q, form="fused", softmax=None, want_attn=False, maps=None):
    """q/k/v flavour.  maps: a list that receives the spatial maps when want_attn"""
    scale = (kq.shape[-1] // heads) ** -0.5
    Qm = q("q", lin(q("a_qk", kq), w, "q", q, "w_qkv") * scale)
    K = q("k", lin(q("a_qk", kq), w, "k", q, "w_qkv"))
    V = q("v", lin(q("a_v", val), w, "v", q, "w_qkv"))
    out, m = core(Qm, K, V, w, T, heads, q, form, softmax, want_attn)
    if maps is not None:
        maps.append(m)
    return out


def cc_traj(x, w, T, heads, q, form="fused", softmax=None):
    """cross-clip flavour (axvs_cc.h): one fused qkv projection of x, no positional term"""
    C = x.shape[-1]
    qkv = lin(q("a_qk", x), w, "qkv", q, "w_qkv")
    return core(q("q", qkv[..., :C] * (C // heads) ** -0.5), q("k", qkv[..., C:2 * C]), q("v", qkv[..., 2 * C:]), w, T, heads, q, form, softmax)[0]


def _two(v):
    return v if isinstance(v, tuple) else (v, v)


def _ffn_tail(x, w, q):
    x = orc._layer_norm(x, w, "norm1")
    ff = lin(q("h", torch.relu(lin(q("y", x), w, "linear1", q, "w_ffn"))), w, "linear2", q, "w_ffn")
    return orc._layer_norm(x + ff, w, "norm2")


def layer(src, pos, w, heads, q, form="fused", softmax=None, maps=None):
    """the axial layer.  q and form: one for both passes, or a (height, width) tuple; the FFN takes the width pass's Q.  maps: a list that
    receives the height and the width pass's spatial maps"""
    (qh, qw), (fh, fw) = _two(q), _two(form)
    want = maps is not None
    B, T, H, W, C = pos.shape
    x = src.reshape(B, T, H, W, C)
    xs = x.permute(0, 3, 1, 2, 4).reshape(B * W, T * H, C)
    ps = pos.permute(0, 3, 1, 2, 4).reshape(B * W, T * H, C)
    xs = xs + traj(xs + ps, xs, orc._sub(w, "height_attn"), T, heads, qh, fh, softmax, want, maps)
    x = xs.reshape(B, W, T, H, C).permute(0, 2, 3, 1, 4)
    xs = x.permute(0, 2, 1, 3, 4).reshape(B * H, T * W, C)
    ps = pos.permute(0, 2, 1, 3, 4).reshape(B * H, T * W, C)
    xs = xs + traj(xs + ps, xs, orc._sub(w, "width_attn"), T, heads, qw, fw, softmax, want, maps)
    x = xs.reshape(B, H, T, W, C).permute(0, 2, 1, 3, 4).reshape(B * T, H * W, C)
    return _ffn_tail(x, w, qw)


def full_layer(src, pos, w, heads, q, form="fused", softmax=None):
    """the full T*H*W layer (orc.trajectory_layer): one trajectory attention over all tokens of a clip, frames of H W keys"""
    B, T = pos.shape[:2]
    C = src.shape[-1]
    x = src.reshape(B, -1, C)
    y = traj(x + pos.reshape(B, -1, C), x, orc._sub(w, "temporal_attn"), T, heads, q, form, softmax)
    return _ffn_tail((x + y).reshape(src.shape), w, q)
