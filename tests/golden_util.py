"""Helpers to replay tests/golden/*.npz (made by oracle/gen_golden.py from the reference)."""
import json
import os

import numpy as np
import torch

import axvs_oracle as orc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    if isinstance(meta.get("shapes"), dict):        # parameter shape table (G7 fixtures keep spatial shapes under this key)
        meta["shapes"] = {k: tuple(v) for k, v in meta["shapes"].items()}
    return z, meta


def weights(z, meta, seed=None):
    """Regenerate the fixture's weights from its seed; verify against the stored checksum."""
    w = orc.random_weights(meta["shapes"], meta["seed"] if seed is None else seed)
    got = float(sum(v.double().sum() for v in w.values()))
    assert abs(got - float(z["wsum"])) < 1e-6 * max(1.0, abs(got)), "torch RNG drift: regenerate fixtures"
    return w


def t(a):
    return torch.from_numpy(np.asarray(a))


def rel_err(a, b):
    """max |a-b| / max |b|  (the parity metric used throughout: error relative to the tensor's scale)."""
    a = a.double()
    b = b.double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


# Element-level parity report (round 6).  `rel_err` scales the largest error by the largest reference magnitude and `rel_l2` averages: neither says how
# single elements fare.  elem_report(a, b) counts the elements outside the band  |a - b| <= scale * (ELEM_RTOL * |b| + ELEM_ATOL_RMS * rms(b))  -- 1e-3 of
# the element's own magnitude plus 1e-3 of the tensor's rms (so that near-zero elements are not asked for 1e-3 of nothing) -- prints the fraction outside
# the band, the fraction outside THREE TIMES the band and the worst ratio, and elem_check bounds both fractions.  What the 16-bit MFMA tier holds
# (measured on the GPU, profiles/r6_element_parity.txt): the rounding errors are ~Gaussian with sigma ~ 0.3 - 0.6 of the band, so between 1e-4 and 9e-2
# of the elements lie outside the 1x band (most on unnormalised outputs and on the free-running six-layer stack) and essentially none outside 3x; every
# element is inside 1x only on the fp32 tier.  Stated bound: <= ELEM_FRAC1 outside the band, <= ELEM_FRAC3 outside three times the band.
ELEM_RTOL = 1e-3
ELEM_ATOL_RMS = 1e-3
ELEM_FRAC1 = 0.10
ELEM_FRAC3 = 1e-3
ELEM_LOG = []


def elem_report(a, b, what="", scale=1.0):
    a = a.double().reshape(-1)
    b = b.double().reshape(-1)
    rms = float(b.pow(2).mean().sqrt())
    band = scale * (ELEM_RTOL * b.abs() + ELEM_ATOL_RMS * rms)
    ratio = (a - b).abs() / band.clamp_min(1e-300)
    f1 = float((ratio > 1.0).double().mean())
    f3 = float((ratio > 3.0).double().mean())
    worst = float(ratio.max())
    ELEM_LOG.append((what, f1, f3, worst))
    print(f"[elem] {what}: {f1:.2e} / {f3:.2e} of {a.numel()} elements outside 1x / 3x the band {scale:g} * ({ELEM_RTOL:g}|b| + {ELEM_ATOL_RMS:g} rms(b)), worst {worst:.2f}x")
    return f1, f3


def elem_check(a, b, what="", tol=1e-3):
    """bound the element-level fractions; `tol` is the max-norm tolerance of the test (the band scales with it: 1e-3 -> scale 1)"""
    f1, f3 = elem_report(a, b, what, scale=tol / 1e-3)
    assert f1 <= ELEM_FRAC1 and f3 <= ELEM_FRAC3, (what, f1, f3)


def rel_l2(a, b):
    a = a.double()
    b = b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def checks(x):
    x = x.double()
    return np.array([x.sum().item(), (x * x).sum().item(), x.abs().max().item()])


def axial_inputs(meta):
    g = torch.Generator().manual_seed(meta["seed"] + 1)
    B, T, C, H, W = (meta[k] for k in "BTCHW")
    x = torch.randn(B, T, C, H, W, generator=g)
    src = x.permute(0, 1, 3, 4, 2).reshape(B * T, H * W, C).contiguous()
    pos = orc.pos_embed_sine_3d(B, T, H, W, C // 2)
    return src, pos


AXIAL = ["g2_axial_B1_T2_C128_H32_W32", "g2_axial_B2_T3_C64_H5_W7", "g2_axial_B1_T5_C64_H6_W4",
         "g2_axial_B1_T1_C64_H4_W5", "g2_axial_B1_T4_C256_H64_W64"]
# reference-generated fixtures at the map sizes the shipped configurations run (oracle/gen_golden_shipped.py, round 5): VIPSeg R50 (T = 2) and
# Tube-Link YouTube-VIS (T = 5) temporal levels -- frame lengths that are not multiples of 16
SHIPPED = ["g15_shipped_B1_T2_C256_H49_W85", "g15_shipped_B1_T2_C256_H25_W43", "g15_shipped_B1_T5_C256_H24_W40", "g15_shipped_B1_T5_C256_H12_W20"]
TRAJ_LAYER = ["g2b_traj_layer_B1_T2_C64_H6_W5", "g2b_traj_layer_B1_T3_C256_H12_W16", "g2b_traj_layer_B2_T2_C256_H20_W24"]
TRAJ = ["g1_traj_S3_T2_L7_C64", "g1_traj_S2_T5_L6_C64", "g1_traj_S2_T1_L9_C64", "g1_traj_S4_T4_L16_C256"]


MSDA_CORE = ["g7_msda_core_N1_M2_D2_Lq2_L2_P2", "g7_msda_core_N2_M8_D32_Lq50_L3_P4", "g7_msda_core_N1_M4_D30_Lq33_L2_P3"]
MSDA_MODULE = ["g7_msda_module_N2_C256_L3_S252", "g7_msda_module_N1_C64_L2_S39", "g7_msda_module_N4_C256_L3_S5376"]


def msda_core_inputs(m):
    """The reference test's input recipe (ops/test.py:36-41), seeded; `spread` pushes locations outside [0,1].  Locations are (x, y),
    normalised to [0, 1] over each level's map: the convention stated once in msda_cases.py."""
    g = torch.Generator().manual_seed(m["seed"])
    shapes, N, M, D, Lq, P, spread = m["shapes"], m["N"], m["M"], m["D"], m["Lq"], m["P"], m["spread"]
    L, S = len(shapes), sum(h * w for h, w in shapes)
    value = torch.rand(N, S, M, D, generator=g) * m.get("scale", 0.01)
    loc = torch.rand(N, Lq, M, L, P, 2, generator=g) * (1 + 2 * spread) - spread
    aw = torch.rand(N, Lq, M, L, P, generator=g) + 1e-5
    aw = aw / aw.sum(-1, keepdim=True).sum(-2, keepdim=True)
    return value, loc, aw


MSDA_BWD = ["g14_msda_bwd_N1_M2_D2_Lq2_L2_P2", "g14_msda_bwd_N2_M8_D32_Lq50_L3_P4", "g14_msda_bwd_N1_M4_D30_Lq33_L2_P3",
            "g14_msda_bwd_N1_M8_D16_Lq40_L1_P5"]


def msda_module_case(z, m):
    """weights + inputs of a G7b fixture: (state dict, query, reference_points, src, padding mask or None)."""
    import axvs_oracle as orc
    w = orc.random_weights({k: tuple(v) for k, v in m["wshapes"].items()}, m["seed"])
    for k in z.files:
        if k.startswith("w."):
            w[k[2:]] = torch.from_numpy(z[k])
    shapes, N, C = m["shapes"], m["N"], m["C"]
    L, S = len(shapes), sum(h * ww for h, ww in shapes)
    g = torch.Generator().manual_seed(m["seed"] + 1)
    for k in ("sampling_offsets.weight", "attention_weights.weight", "attention_weights.bias"):   # the generator's draw order
        torch.rand(w[k].shape, generator=g)
    src = torch.randn(N, S, C, generator=g)
    pos = torch.randn(N, S, C, generator=g) * 0.5
    refs = []
    for (h, ww) in shapes:
        ys, xs = torch.meshgrid(torch.linspace(0.5, h - 0.5, h) / h, torch.linspace(0.5, ww - 0.5, ww) / ww, indexing="ij")
        refs.append(torch.stack([xs.reshape(-1), ys.reshape(-1)], -1))
    ref = torch.cat(refs, 0)[None, :, None, :].expand(N, S, L, 2).contiguous()
    pm = None
    if m["mask"]:
        pm = torch.zeros(N, S, dtype=torch.bool)
        pm[0, 5:40] = True
        pm[1, -7:] = True
    return w, src + pos, ref, src, pm


MSDA_ENCLAYER = ["g7_msda_enclayer_N2_C256_L3_S252", "g7_msda_enclayer_N1_C64_L2_S39"]


def msda_enclayer_case(z, m):
    """weights + inputs of a G7c fixture: (state dict, src, pos, reference_points, padding mask or None)."""
    import axvs_oracle as orc
    w = orc.random_weights({k: tuple(v) for k, v in m["wshapes"].items()}, m["seed"])
    for k in z.files:
        if k.startswith("w."):
            w[k[2:]] = torch.from_numpy(z[k])
    shapes, N, C = m["shapes"], m["N"], m["C"]
    L, S = len(shapes), sum(h * ww for h, ww in shapes)
    g = torch.Generator().manual_seed(m["seed"] + 1)
    for k in ("self_attn.sampling_offsets.weight", "self_attn.attention_weights.weight", "self_attn.attention_weights.bias"):
        torch.rand(w[k].shape, generator=g)
    src = torch.randn(N, S, C, generator=g)
    pos = torch.randn(N, S, C, generator=g) * 0.5
    refs = []
    for (h, ww) in shapes:
        ys, xs = torch.meshgrid(torch.linspace(0.5, h - 0.5, h) / h, torch.linspace(0.5, ww - 0.5, ww) / ww, indexing="ij")
        refs.append(torch.stack([xs.reshape(-1), ys.reshape(-1)], -1))
    ref = torch.cat(refs, 0)[None, :, None, :].expand(N, S, L, 2).contiguous()
    pm = None
    if m["mask"]:
        pm = torch.zeros(N, S, dtype=torch.bool)
        pm[0, 5:40] = True
        pm[1, -7:] = True
    return w, src, pos, ref, pm


TL_PLUGIN = ["g9_tl_plugin_T2_L3_l1", "g9_tl_plugin_T3_L3_l2", "g9_tl_plugin_T4_L2_l1"]


def tl_plugin_case(z, m, C=256):
    """weights + inputs of a G9 fixture (same recipe as oracle/gen_golden_tl_plugin.py:plugin_case / scale_gamma), batch-first:
    (state dict, query, query_pos, pos3d list, reference_points, key_padding_mask or None)."""
    import axvs_oracle as orc
    w = orc.random_weights({k: tuple(v) for k, v in m["wshapes"].items()}, m["seed"])
    if "gamma" in w:
        w["gamma"] = w["gamma"] * 10.0 + 1.0
    assert abs(sum(v.double().sum().item() for v in w.values()) - float(z["wsum"])) < 1e-6 * max(1.0, abs(float(z["wsum"])))
    g = torch.Generator().manual_seed(m["seed"] + 1)
    B, T, shapes = m["B"], m["T"], [tuple(s) for s in m["shapes"]]
    bs, nq = B * T, sum(h * ww for h, ww in shapes)
    query = torch.randn(bs, nq, C, generator=g)
    query_pos = torch.randn(bs, nq, C, generator=g) * 0.5
    lvl3d = torch.randn(m["temporal_levels"], C, generator=g) * 0.3
    pos3d = [orc.pos_embed_sine_3d(B, T, h, ww, C // 2) + lvl3d[i].view(1, 1, 1, 1, -1)
             for i, (h, ww) in enumerate(shapes[:m["temporal_levels"]])]
    refs = []
    for (h, ww) in shapes:
        ys, xs = torch.meshgrid((torch.arange(h) + 0.5) / h, (torch.arange(ww) + 0.5) / ww, indexing="ij")
        refs.append(torch.stack([xs.reshape(-1), ys.reshape(-1)], -1))
    ref = torch.cat(refs, 0)[None, :, None].repeat(bs, 1, len(shapes), 1)
    mask = (torch.rand(bs, nq, generator=g) < 0.1) if m["mask"] else None
    return w, query, query_pos, pos3d, ref, mask


TRAIN = ["g10_train_B1_T2_C64_H5_W6", "g10_train_B2_T3_C64_H4_W5", "g10_train_B1_T2_C256_H8_W8", "g10_train_B1_T4_C128_H6_W3"]


def train_inputs(meta, dtype=torch.float64):
    """(src, pos, d_out) of a g10 fixture (oracle/gen_golden_train.py)."""
    g = torch.Generator().manual_seed(meta["seed"] + 1)
    B, T, C, H, W = (meta[k] for k in "BTCHW")
    x = torch.randn(B, T, C, H, W, generator=g)
    src = x.permute(0, 1, 3, 4, 2).reshape(B * T, H * W, C).contiguous().to(dtype)
    pos = orc.pos_embed_sine_3d(B, T, H, W, C // 2).to(dtype)
    d_out = torch.randn(B * T, H * W, C, generator=g).to(dtype)
    return src, pos, d_out


def train_grad_errors(z, grads):
    """Error of every parameter gradient {name: tensor} against a g10 fixture (full arrays, or every 5th element + checksums):
    |got - ref|_2 / max(|ref|_2, 1e-3 * the largest gradient norm of the layer).  The floor matters for k.bias only: the key bias
    cancels in the softmax, its true gradient is 0 and both sides hold rounding noise."""
    names = list(grads)
    refs = {k: t(z["grad." + k]).double() for k in names}
    floor = 1e-3 * max(float(np.sqrt(np.asarray(z["gradchk." + k])[1])) for k in names)
    errs = {}
    for k in names:
        ref = refs[k]
        got = grads[k].detach().cpu().double()
        if ref.numel() != got.numel():
            refc = np.asarray(z["gradchk." + k])
            errs[k + ":sumsq"] = abs(checks(got)[1] - refc[1]) / max(refc[1], floor * floor)
            got = got.reshape(-1)[::5]
        errs[k] = float((got.reshape(-1) - ref.reshape(-1)).norm() / max(float(ref.norm()), floor))
    return errs


CC_TRAIN = ["g13_cc_train_B1_Q16_Tc3_V2_H8_L2", "g13_cc_train_B1_Q16_Tc4_V2_H8_L2", "g13_cc_train_B2_Q8_Tc2_V1_H4_L1",
            "g13_cc_train_B1_Q24_Tc5_V1_H8_L3", "g13_cc_train_B1_Q8_Tc12_V1_H5_L1", "g13_cc_train_B1_Q16_Tc2_V2_H3_L2"]


def cc_train_inputs(m):
    g = torch.Generator().manual_seed(m["seed"] + 1)
    cq = torch.randn(m["B"], m["Q"], m["Tc"], 256, generator=g)
    pf = torch.nn.functional.normalize(torch.randn(m["B"], 128, m["Tc"] * m["V"], m["H"], m["W"], generator=g), dim=1)
    return cq, pf


POS_MASK = ["g11_pos3d_mask_B2_T3_H6_W7_n16", "g11_pos3d_mask_B1_T4_H12_W9_n64", "g11_pos3d_mask_B2_T2_H5_W8_n32"]
GELU = ["g12_axial_gelu_B1_T2_C64_H6_W5", "g12_axial_gelu_B1_T3_C256_H16_W16"]
