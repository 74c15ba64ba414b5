"""The within-clip training tier (axvs_train.h, axvs_train_host.h, training.py) at its tier edges and at T up to 16: the case table,
weights, inputs, float64 reference and error measures shared by tests/test_traj_train_cases_cpu.py and
tests/test_hip_traj_train_cases.py.  Everything runs through TemporalAxialTrajectoryAttentionLayer ("axial") and
TemporalTrajectoryAttentionLayer ("full") in train() mode.

REFERENCE.  oracle/axvs_oracle.py::axial_layer_train and `traj_layer_train_ref` below (the full layer, composed from
orc.trajectory_attention and the hash dropout of include/axvs.h, sites 1, 2, 5, 6) in float64 under torch.autograd.  The same function
in float32 is the yardstick of the ratio r below.

WEIGHTS AND INPUTS.  orc.random_weights over the layer's parameter shapes, orc.synthetic_clip, d_out ~ N(0, 1), all from the case's
seed: the recipe of the float64 tests in test_hip_training.py and test_hip_traj_training.py.

ERROR MEASURES (those of the two files).  out, d_src, d_pos: max|got - ref| / max|ref| (rel_err) and |got - ref|_2 / |ref|_2 (rel_l2).
A parameter gradient: |got - ref|_2 / max(|ref|_2, 1e-3 * the largest gradient norm of the layer).

THE RATIO r of a tensor = max|device - f64| / max(max|oracle fp32 - f64|, 2^-24 max|f64|): how far the device is from float64 in units
of what plain fp32 torch is; the floor is one rounding of an fp32 result (as in cc_train_cases.py).

GRADIENTS THAT VANISH IN EXACT ARITHMETIC (`vanishing`): every pass's k.bias (a softmax ignores a common shift of its logits); at T = 1
each pass's proj_q.weight and proj_q.bias (the temporal softmax runs over one frame); at L = 1 that pass's q.weight, q.bias and k.weight
(the spatial softmax runs over one key).  Both sides hold rounding noise there, so they are held to an absolute bound.

RELU MARGIN.  The FFN's ReLU makes the gradients discontinuous in the forward: a hidden unit whose pre-activation lies within fp32
rounding of zero can land on the other side in an fp32 forward, and that unit's mask then moves d_src by ~1e-2 at one token (a tie,
not an error).  `reference` returns the smallest margin of a case, min over hidden units of |pre-activation| / sum_c |z_c w_fc|, from
float64; the CPU test holds it above 2^-21, eight fp32 roundings of the sum's terms.

WHAT EACH CASE REACHES is derived from the host code next to it in CASES; `structure` restates those host formulas (spatial_tier, the
LDS sizes, spatial_grid, spatial_kv_chunk, chunk_tiles, the VALU kernels' outer loops, the temporal kernels' TMAX, Ctx::colsum's block
plan) and the CPU test asserts each claim, so the table cannot drift from its comments."""
import contextlib
import math
from collections import namedtuple

import torch

import axvs_oracle as orc
from golden_util import rel_err, rel_l2

TOL = 1e-4          # the bar of test_hip_training.py and test_hip_traj_training.py
FLOOR = 2.0 ** -24
RELU_MARGIN = 2.0 ** -21
VANISH_NOISE = 1e-7                 # of the largest gradient norm: what fp32 torch may leave on a gradient that is zero in exact arithmetic

# the host's constants (axvs_train.h, axvs_train_host.h, axvs_host.h)
K_TR_LD, K_SP_MAX_TILES, K_SP_CHUNK, K_SP_QT, K_MAX_LDS, K_SPATIAL_WGS, K_COLSUM_BLOCKS, K_VALU_QC = 36, 8, 256, 2, 160 * 1024, 512, 512, 32
LDS_DEFAULT = 64 * 1024             # above it Ctx::launch_lds raises the kernel's limit

Case = namedtuple("Case", "kind B T C heads H W F p_dropout p_attn_drop seed valu")

# (S, N, L) of a pass: the two axial passes have (B W, T H, H) and (B H, T W, W); the full layer (B, T HW, HW).  Claims are keyed
# "<pass>.<key>" with pass h (height), w (width) or t (the full layer's one pass).
CASES = {
    # width pass N = 16 * 33 = 528 > 512: spatial_kv_chunk gives Nc = 512, two query chunks, the second with 16 live rows and no padding;
    # T = 16: TMAX 16, spatial_grid z = 16 (sh = 24); L = 33: Split with a third key tile of 1 key; height pass L = 3
    "axial_t16_kv_two_chunks": Case("axial", 1, 16, 256, 8, 3, 33, 64, 0.1, 0.1, 4000, 0),
    # N = 9 * 57 = 513: the second chunk holds 1 live query and 15 padding rows (1 / sum = 0); T = 9, the smallest TMAX-16
    "axial_t9_kv_one_live": Case("axial", 1, 9, 256, 8, 2, 57, 64, 0.0, 0.0, 4000, 0),
    # height pass L = 128: Split with all kSpMaxTiles register tiles; width pass L = 129: Mfma, a ninth tile of 1 key; both key-side
    # launches above 64 KiB; M = 33024 rows: colsum rpb = 65, 509 blocks, the last of 4 rows.  F = 8: 264 k hidden units (ReLU margin)
    "axial_split128_mfma129": Case("axial", 1, 2, 64, 2, 128, 129, 8, 0.1, 0.1, 4001, 0),
    # width pass sh = 64 * 8 = 512 = g_spatial_wgs: grid (512, 1, 1), one workgroup walks the 3 frames and a wave a second query tile
    # (5 tiles on 4 waves); height pass sh = 368: the split grid
    "axial_one_wg_per_seq": Case("axial", 2, 3, 256, 8, 32, 23, 64, 0.0, 0.0, 4000, 0),
    # height pass L = 1 (H = 1): a softmax over one key
    "axial_l1": Case("axial", 1, 3, 256, 8, 1, 17, 64, 0.1, 0.1, 4000, 0),
    # T = 1 on Split (head_dim 32) and on VALU (head_dim 8)
    "axial_t1": Case("axial", 2, 1, 256, 8, 5, 4, 64, 0.0, 0.0, 4000, 0),
    "axial_t1_d8": Case("axial", 2, 1, 64, 8, 5, 4, 64, 0.1, 0.1, 4000, 0),
    # T = 8: TMAX 8 with every slot live
    "axial_t8": Case("axial", 1, 8, 256, 8, 3, 5, 64, 0.0, 0.0, 4000, 0),
    # head_dim 64, T = 7: the VALU key-side kernel's lds_kv = (32 * 64 + 32 * 7 * 64 + 32 * 7 * 3) * 4 = 68224 B, above 64 KiB
    "axial_d64_t7": Case("axial", 1, 7, 128, 2, 4, 5, 64, 0.1, 0.1, 4000, 0),
    # the same at T = 16: 145408 B; the <64, 16> temporal kernels
    "axial_d64_t16": Case("axial", 1, 16, 128, 2, 3, 2, 64, 0.0, 0.0, 4000, 0),
    # the <8, 16> and <16, 16> temporal kernels
    "axial_d8_t9": Case("axial", 1, 9, 64, 8, 3, 4, 64, 0.1, 0.1, 4000, 0),
    "axial_d16_t16": Case("axial", 1, 16, 128, 8, 2, 3, 64, 0.0, 0.0, 4000, 0),
    # head_dim 16, N = 3 * 99 = 297: the VALU kernels' outer loops take a second iteration with 41 live threads; in
    # tr_spatial_bwd_kv_kernel those are keys 256 .. 296, all of frame 2 (f = kn / L)
    "full_valu_n297": Case("full", 1, 3, 128, 8, 9, 11, 64, 0.1, 0.1, 4000, 0),
    # head_dim 64, L = 143: the VALU query-side kernels hold 2 * 143 * 64 * 4 = 73216 B > 64 KiB; N = 286
    "full_d64_l143": Case("full", 1, 2, 128, 2, 13, 11, 64, 0.0, 0.0, 4000, 0),
    # head_dim 64, L = 320: 163840 B = kMaxLds exactly, the longest frame check_frame lets through; T = 1
    "full_d64_l320": Case("full", 1, 1, 128, 2, 16, 20, 64, 0.1, 0.1, 4000, 0),
    # the Split / Mfma boundary without the big M
    "full_split128": Case("full", 1, 2, 64, 2, 8, 16, 64, 0.0, 0.0, 4000, 0),
    "full_mfma129": Case("full", 1, 2, 64, 2, 3, 43, 64, 0.1, 0.1, 4000, 0),
    # L = 560: the last LDS-resident frame (161280 B); N = 1120: three query chunks (512, 512, 96)
    "full_mfma560": Case("full", 1, 2, 64, 2, 20, 28, 64, 0.0, 0.0, 4000, 0),
    # L = 561: the first Chunk frame, key chunks 256 / 256 / 49; nqt = 71 against 9 blocks of 8 tiles: one (wave, u) slot idle
    "full_chunk561": Case("full", 1, 2, 64, 2, 17, 33, 64, 0.1, 0.1, 4000, 0),
    # L = 769: the last key chunk holds 1 key
    "full_chunk769": Case("full", 1, 2, 64, 2, 1, 769, 64, 0.0, 0.0, 4000, 0),
    # axial_t16_kv_two_chunks with option train_valu: the <32> VALU kernels past 256 queries / keys (three iterations, 16 live threads
    # in the last), their key-side launch above 64 KiB at T = 16
    "mfma_as_valu": Case("axial", 1, 16, 256, 8, 3, 33, 64, 0.1, 0.1, 4000, 1),
}
TWICE = ("axial_t9_kv_one_live", "full_valu_n297")      # run twice on the device, identical bits required (fixed summation orders)

# what the comments above claim, per case: the CPU test compares this with structure(case)
CLAIMS = {
    "axial_t16_kv_two_chunks": {"w.N": 528, "w.L": 33, "w.tier": "Split", "w.Nc": 512, "w.nchunks": 2, "w.last_chunk_live": 16, "w.last_chunk_pad": 0,
                                "TMAX": 16, "w.grid_fwd": (24, 2, 16), "w.grid_bwd_kv": (24, 1, 16), "w.last_tile_keys": 1, "h.L": 3},
    "axial_t9_kv_one_live": {"w.N": 513, "w.Nc": 512, "w.nchunks": 2, "w.last_chunk_live": 1, "w.last_chunk_pad": 15, "TMAX": 16, "T": 9},
    "axial_split128_mfma129": {"h.L": 128, "h.tier": "Split", "h.nkt": 8, "w.L": 129, "w.tier": "Mfma", "w.nkt": 9, "w.last_tile_keys": 1,
                               "h.lds_bwd_kv": 77824, "w.lds_bwd_kv": 82688, "h.kv_over_64k": True, "w.kv_over_64k": True,
                               "M": 33024, "colsum": (65, 509, 4)},
    "axial_one_wg_per_seq": {"w.sh": 512, "w.grid_fwd": (512, 1, 1), "w.grid_bwd_q": (512, 1, 1), "w.grid_bwd_kv": (512, 1, 1),
                             "w.frames_per_wg": 3, "w.nqt": 5, "w.qtiles_per_wave": 2, "h.sh": 368, "h.grid_fwd": (368, 1, 3)},
    "axial_l1": {"h.L": 1, "h.tier": "Split", "T": 3},
    "axial_t1": {"T": 1, "h.tier": "Split", "w.tier": "Split", "TMAX": 8},
    "axial_t1_d8": {"T": 1, "D": 8, "h.tier": "Valu", "w.tier": "Valu"},
    "axial_t8": {"T": 8, "TMAX": 8},
    "axial_d64_t7": {"D": 64, "T": 7, "h.tier": "Valu", "h.lds_bwd_kv": 68224, "w.lds_bwd_kv": 68224, "h.kv_over_64k": True, "h.q_over_64k": False},
    "axial_d64_t16": {"D": 64, "TMAX": 16, "h.lds_bwd_kv": 145408, "h.kv_over_64k": True},
    "axial_d8_t9": {"D": 8, "T": 9, "TMAX": 16},
    "axial_d16_t16": {"D": 16, "T": 16, "TMAX": 16},
    "full_valu_n297": {"D": 16, "t.tier": "Valu", "t.N": 297, "t.L": 99, "t.valu_iters": 2, "t.valu_last_live": 41, "t.valu_last_frames": (2,)},
    "full_d64_l143": {"D": 64, "t.L": 143, "t.N": 286, "t.lds_fwd": 73216, "t.q_over_64k": True, "t.valu_iters": 2},
    "full_d64_l320": {"D": 64, "t.L": 320, "t.lds_fwd": K_MAX_LDS, "T": 1, "t.valu_iters": 2},
    "full_split128": {"t.L": 128, "t.tier": "Split", "t.nkt": 8, "M": 256},
    "full_mfma129": {"t.L": 129, "t.tier": "Mfma", "t.nkt": 9, "t.last_tile_keys": 1, "M": 258},
    "full_mfma560": {"t.L": 560, "t.tier": "Mfma", "t.lds_fwd": 161280, "t.N": 1120, "t.nchunks": 3, "t.last_chunk_live": 96},
    "full_chunk561": {"t.L": 561, "t.tier": "Chunk", "t.key_chunks": 3, "t.last_key_chunk": 49, "t.nqt": 71, "t.chunk_tiles": 36, "t.idle_slots": 1},
    "full_chunk769": {"t.L": 769, "t.tier": "Chunk", "t.key_chunks": 4, "t.last_key_chunk": 1},
    "mfma_as_valu": {"D": 32, "w.tier": "Valu", "w.N": 528, "w.valu_iters": 3, "w.valu_last_live": 16, "w.lds_bwd_kv": 75776, "w.kv_over_64k": True,
                     "w.grid_fwd": (24, 1, 1)},
}


def ceil16(n):
    return (n + 15) // 16 * 16


def passes(c):
    """[(pass key, parameter prefix, S, N, L)] in the order the forward runs them"""
    if c.kind == "axial":
        return [("h", "height_attn", c.B * c.W, c.T * c.H, c.H), ("w", "width_attn", c.B * c.H, c.T * c.W, c.W)]
    return [("t", "temporal_attn", c.B, c.T * c.H * c.W, c.H * c.W)]


def spatial_frame_lds(L):
    return 2 * ceil16(L) * K_TR_LD * 4


def spatial_split_lds(L):
    Lp = ceil16(L)
    return 3 * (Lp * 32 + 32 * (Lp + 4)) * 2


def spatial_chunk_lds():
    return 2 * K_SP_CHUNK * K_TR_LD * 4


def spatial_kv_lds(Nc):
    return Nc * (2 * K_TR_LD + 4) * 4


def spatial_tier(D, L, valu, split=True):
    if D != 32 or valu:
        return "Valu"
    if spatial_frame_lds(L) > K_MAX_LDS:
        return "Chunk"
    return "Split" if split and L <= 16 * K_SP_MAX_TILES else "Mfma"


def spatial_grid(sh, tiles, frames):
    if sh >= K_SPATIAL_WGS:
        return (sh, 1, 1)
    y = -(-K_SPATIAL_WGS // (sh * frames))
    return (sh, max(1, min(y, (tiles + 3) // 4)), frames)


def pass_structure(c, S, N, L):
    """one pass's launches: spatial_fwd and spatial_bwd restated"""
    D, T = c.C // c.heads, c.T
    sh, nqt, nkt = S * c.heads, -(-N // 16), -(-L // 16)
    tier = spatial_tier(D, L, c.valu)
    s = dict(S=S, N=N, L=L, sh=sh, nqt=nqt, nkt=nkt, last_tile_keys=L - (nkt - 1) * 16, tier=tier)
    none = dict(Nc=None, nchunks=None, last_chunk_live=None, last_chunk_pad=None, chunk_tiles=None, idle_slots=None, key_chunks=None,
                last_key_chunk=None, valu_iters=None, valu_last_live=None, valu_last_frames=None)
    s.update(none)
    if tier == "Valu":
        lds_q = 2 * L * D * 4                                            # spatial_valu_lds
        s.update(lds_fwd=lds_q, lds_bwd_q=lds_q, lds_bwd_kv=(K_VALU_QC * D + K_VALU_QC * T * D + K_VALU_QC * T * 3) * 4,
                 grid_fwd=(sh, 1, 1), grid_bwd_q=(sh, 1, 1), grid_bwd_kv=(sh, 1, 1), frame_fits=lds_q <= K_MAX_LDS)
        iters = -(-N // 256)                                             # for (q0 = 0; q0 < N; q0 += 256), and k0 alike
        first = (iters - 1) * 256
        s.update(valu_iters=iters, valu_last_live=N - first, valu_last_frames=tuple(sorted({kn // L for kn in range(first, N)})))
    else:
        Nc = min(ceil16(N), 512)                                         # spatial_kv_chunk
        nchunks = -(-ceil16(N) // Nc)
        live = N - (nchunks - 1) * Nc
        s.update(Nc=Nc, nchunks=nchunks, last_chunk_live=live, last_chunk_pad=min(Nc, ceil16(N) - (nchunks - 1) * Nc) - live,
                 lds_bwd_kv=spatial_kv_lds(Nc), grid_bwd_kv=spatial_grid(sh, nkt, T), frame_fits=True)
        if tier == "Chunk":
            nqb = -(-nqt // (4 * K_SP_QT))
            ct = nqb * 4                                                 # chunk_tiles
            kc = -(-L // K_SP_CHUNK)
            s.update(lds_fwd=spatial_chunk_lds(), lds_bwd_q=spatial_chunk_lds(), grid_fwd=spatial_grid(sh, ct, T), grid_bwd_q=spatial_grid(sh, ct, 1),
                     chunk_tiles=ct, idle_slots=nqb * 4 * K_SP_QT - nqt, key_chunks=kc, last_key_chunk=L - (kc - 1) * K_SP_CHUNK)
        else:
            s.update(lds_fwd=spatial_split_lds(L) if tier == "Split" else spatial_frame_lds(L), lds_bwd_q=spatial_frame_lds(L),
                     grid_fwd=spatial_grid(sh, nqt, T), grid_bwd_q=spatial_grid(sh, nqt, 1))
    s["q_over_64k"] = max(s["lds_fwd"], s["lds_bwd_q"]) > LDS_DEFAULT
    s["kv_over_64k"] = s["lds_bwd_kv"] > LDS_DEFAULT
    gx, gy, gz = s["grid_fwd"]
    s["frames_per_wg"] = -(-T // gz)                                     # frames one forward workgroup walks
    s["qtiles_per_wave"] = -(-nqt // (4 * gy)) if tier != "Valu" else None
    return s


def structure(c):
    """The host's branch and plan arithmetic for a case, restated: flat {key: value}, a pass's keys prefixed "h.", "w." or "t."."""
    D, M = c.C // c.heads, c.B * c.T * c.H * c.W
    rpb = max(-(-M // K_COLSUM_BLOCKS), 64)                              # Ctx::colsum
    nblk = -(-M // rpb)
    out = dict(D=D, M=M, T=c.T, TMAX=8 if c.T <= 8 else 16, colsum=(rpb, nblk, M - (nblk - 1) * rpb), hidden_units=M * c.F)
    for key, _, S, N, L in passes(c):
        out.update({f"{key}.{k}": v for k, v in pass_structure(c, S, N, L).items()})
    return out


def accepted(c):
    """make_dims_any, make_dims (axial) / check_frame (every VALU pass) let the shape through"""
    D = c.C // c.heads
    M = c.B * c.T * c.H * c.W
    ok = c.C % c.heads == 0 and D in (8, 16, 32, 64) and c.F % 8 == 0 and 1 <= c.T <= 16 and M * max(c.T, 1) <= 2 ** 31 - 1
    if c.kind == "axial":
        ok = ok and 2 * max(c.H, c.W) * D * 4 <= 160 * 1024
    st = structure(c)
    return ok and all(st[f"{key}.frame_fits"] for key, *_ in passes(c))


def param_shapes(c):
    shapes = orc.axial_layer_param_shapes(c.C, c.F)
    if c.kind == "full":
        shapes = {k.replace("height_attn", "temporal_attn"): v for k, v in shapes.items() if "width_attn" not in k}
    return shapes


def make_weights(c):
    return orc.random_weights(param_shapes(c), c.seed)


def make_inputs(c):
    """(src [(B T), HW, C], pos [B, T, H, W, C], d_out like src), fp32"""
    src, pos = orc.synthetic_clip(c.B, c.T, c.C, c.H, c.W, c.seed)
    d_out = torch.randn(c.B * c.T, c.H * c.W, c.C, generator=torch.Generator().manual_seed(c.seed + 1))
    return src, pos, d_out


def dropout_seed(c):
    return c.seed + 31337


def traj_layer_train_ref(src, pos, w, heads, p_drop, p_attn, seed):
    """TemporalTrajectoryAttentionLayer.forward in train() mode with the tier's dropout factors: differentiable torch code."""
    B, T = pos.shape[:2]
    C = src.shape[-1]
    dt = src.dtype
    x = src.reshape(B, -1, C)
    N = x.shape[1]
    L = N // T
    keep = orc.dropout_keep(seed, 1, B * heads * N * T * L, p_drop, dt).reshape(B, heads, N, T, L) if p_drop > 0 else None
    kq = x + pos.reshape(B, -1, C).to(dt)
    y, _ = orc.trajectory_attention(kq, kq, x, orc._sub(w, "temporal_attn"), T, heads, want_attn=False, attn_keep=keep)
    x = x + y * orc.dropout_keep(seed, 2, B * N * C, p_attn, dt).reshape(B, N, C)
    z = orc._layer_norm(x.reshape(src.shape), w, "norm1")
    F_ = w["linear1.weight"].shape[0]
    M = B * N
    r = torch.relu(orc._linear(z, w, "linear1")) * orc.dropout_keep(seed, 5, M * F_, p_drop, dt).reshape(*src.shape[:2], F_)
    ff = orc._linear(r, w, "linear2") * orc.dropout_keep(seed, 6, M * C, p_drop, dt).reshape(src.shape)
    return orc._layer_norm(z + ff, w, "norm2")


@contextlib.contextmanager
def _tap_norm1(store):
    """keeps norm1's output (the FFN's input z) of the oracle's forward: both reference functions call orc._layer_norm(x, w, "norm1")"""
    real = orc._layer_norm

    def tapped(x, w, name, *a, **kw):
        y = real(x, w, name, *a, **kw)
        if name == "norm1":
            store["z"] = y.detach()
        return y

    orc._layer_norm = tapped
    try:
        yield
    finally:
        orc._layer_norm = real


def relu_margin(z, w):
    """min over (token, hidden unit) of |pre-activation| / sum_c |z_c w_fc|"""
    z = z.reshape(-1, z.shape[-1])
    W, b = w["linear1.weight"].detach(), w["linear1.bias"].detach()
    return float(((z @ W.t() + b).abs() / (z.abs() @ W.abs().t())).min())


_refs = {}


def reference(case, dtype=torch.float64):
    """One training step of the oracle in `dtype` -> dict: out, d_src, d_pos, grads {name: tensor}, relu_margin.  Computed once per
    (case, dtype) and shared: leave it unchanged."""
    key = (case, dtype)
    if key not in _refs:
        c = CASES[case]
        src, pos, d_out = make_inputs(c)
        wd = {k: v.to(dtype).requires_grad_(True) for k, v in make_weights(c).items()}
        s, p = src.to(dtype).requires_grad_(True), pos.to(dtype).requires_grad_(True)
        fn = orc.axial_layer_train if c.kind == "axial" else traj_layer_train_ref
        tap = {}
        with _tap_norm1(tap):
            out = fn(s, p, wd, c.heads, c.p_dropout, c.p_attn_drop, dropout_seed(c))
        out.backward(d_out.to(dtype))
        _refs[key] = dict(out=out.detach(), d_src=s.grad, d_pos=p.grad, grads={k: v.grad for k, v in wd.items()},
                          relu_margin=relu_margin(tap["z"], wd))
    return _refs[key]


def vanishing(c):
    """the parameter gradients that are zero in exact arithmetic, from the structure alone (sorted names)"""
    names = []
    for _, prefix, _, _, L in passes(c):
        names.append(f"{prefix}.k.bias")
        if c.T == 1:
            names += [f"{prefix}.proj_q.weight", f"{prefix}.proj_q.bias"]
        if L == 1:
            names += [f"{prefix}.q.weight", f"{prefix}.q.bias", f"{prefix}.k.weight"]
    return sorted(names)


def tensors(res):
    """the flat {label: tensor} view of a result dict"""
    out = dict(out=res["out"], d_src=res["d_src"], d_pos=res["d_pos"])
    out.update({"grad." + k: v for k, v in res["grads"].items()})
    return out


def grad_scale(ref):
    return max(float(v.double().norm()) for v in ref["grads"].values())


def errors(got, ref):
    """every measure of `got` against `ref` -> {label: error}, each to be held under TOL (the caller takes the vanishing set out)"""
    e = {}
    for k in ("out", "d_src", "d_pos"):
        e[k] = rel_err(got[k], ref[k])
        e[k + "_l2"] = rel_l2(got[k], ref[k])
    floor = 1e-3 * grad_scale(ref)
    for k, v in ref["grads"].items():
        e["grad." + k] = float((got["grads"][k].double() - v.double()).norm() / max(float(v.double().norm()), floor))
    return e


def ratios(got, ref64, ref32):
    """per tensor: (r, max|got - f64|, yard), r = max|got - f64| / yard, yard = max(max|fp32 oracle - f64|, 2^-24 max|f64|); a tensor
    that is exactly zero in float64 (yard 0) has r = 0 when the device has an exact zero too, else inf"""
    g, a, b = tensors(got), tensors(ref64), tensors(ref32)
    out = {}
    for k in g:
        x = a[k].double()
        yard = max(float((b[k].double() - x).abs().max()), FLOOR * float(x.abs().max()))
        dev = float((g[k].double().cpu() - x).abs().max())
        out[k] = ((dev / yard if yard > 0 else (0.0 if dev == 0 else math.inf)), dev, yard)
    return out


def all_finite(res):
    return all(bool(torch.isfinite(v).all()) for v in tensors(res).values())
