"""The inference planner (plan_traj / plan_ffn in csrc/axvs_api.hip) at every kernel form it can choose: the case table, inputs,
float64 reference and runner shared by tests/test_hip_infer_plan.py and tools/infer_plan_record.py.

A case is one eval-mode forward.  Its kind says what runs:
  "axial"  TemporalAxialTrajectoryAttentionLayer(C, F) on a [B, T, H, W, C] clip (extras: activation, out_dtype, return_attn,
           sine = positions made by PositionEmbeddingSine3D, in_place = the level sits inside a token buffer of that many rows per frame)
  "full"   TemporalTrajectoryAttentionLayer: frames of H * W keys
  "ffn"    axvs_ffn_fwd on H rows (B = T = W = 1)
  "cc"     CrossClipTrackingModule with one layer on [B, Q = H, Tc = T] clip queries
`options` are set on the library around the forward.  All cases have 8 heads.

STAGES holds, per case, the stage names (axvs_profile_stage_name) the library reported BEFORE the planner was stated once -- recorded
from that library by tools/infer_plan_record.py, never from the code under test.  Stage names do not show the tile rows or the merged
form (MQ); profiles/infer_plan_launches_*.txt has the kernel launches per case for those.

What each case is there to reach is the comment next to it; profiles/infer_plan_refactor.md lists which form each one did reach."""
from collections import namedtuple

import torch

import axvs_oracle as orc

SEED = 51
Case = namedtuple("Case", "kind B T C H W F options extras")


def _c(kind, B, T, C, H, W, F=1024, options=(), **extras):
    return Case(kind, B, T, C, H, W, F, tuple(options), extras)


BASE = (1, 2, 256, 64, 64)
CASES = {
    # 64-row tiles, merged MQ = 2 (a row tile is a frame); the FFN rides in the width pass
    "mq2_ffn_rides": _c("axial", *BASE),
    # ... and writes a 16-bit output map
    "mq2_ffn_rides_f16_out": _c("axial", *BASE, out_dtype=torch.float16),
    # 64-row tiles, merged MQ = 1, frames of 32 and 48 keys
    "mq1_frames_32_48": _c("axial", 1, 4, 256, 32, 48),
    # exactly 65 tiles of real rows: the first shape on the 64-row forms; frames padded 40 -> 48 and 52 -> 64 (MQ = 2 on a padded frame)
    "first_on_64_rows": _c("axial", 1, 2, 256, 40, 52),
    # 4080 rows: the last shape whose FFN stays off the width pass (real rows decide: one-chunk split FFN) -- on 64-row tiles all the same
    # (padded rows decide: 102 and 80 tiles)
    "last_on_few_rows": _c("axial", 1, 2, 256, 40, 51),
    # exactly 64 tiles of padded rows in both passes: the last shape on 16-row tiles (256 of them per pass: two launches)
    "last_on_16_rows": _c("axial", 1, 2, 256, 32, 64),
    # 16-row tiles, merged (64 tiles); one-chunk split FFN
    "rows16_merged": _c("axial", 1, 4, 256, 16, 16),
    # 16-row tiles, two launches (256 tiles); 3-way split q/k/v grid
    "rows16_two_launches": _c("axial", 1, 4, 256, 32, 32),
    # ragged frames on 16-row tiles, two launches
    "rows16_ragged": _c("axial", 1, 2, 256, 25, 43),
    # 32-row tiles, merged within one round of the chip; two-chunk split FFN (75 tiles)
    "rows32_merged_split2": _c("axial", 1, 5, 256, 24, 40),
    # 32-row tiles, two launches; stand-alone fused FFN
    "rows32_two_launches": _c("axial", 1, 6, 256, 32, 48, 512),
    # T = 9 .. 12 on 16-row tiles
    "t9_rows16": _c("axial", 1, 9, 256, 16, 16, 512),
    # attention maps: generic spatial half + fused temporal half (NKS = 0)
    "maps_temporal_fused": _c("axial", 1, 2, 256, 16, 12, return_attn=True),
    # generic tier, reassociated temporal half -- and not reassociated
    "t13_reassoc": _c("axial", 1, 13, 256, 8, 8, 256),
    "t13_no_reassoc": _c("axial", 1, 13, 256, 8, 8, 256, [("plan_force", 64)]),
    # generic GEMMs, generic FFN (LayerNorm / GEMM / GEMM / LayerNorm)
    "generic_c64": _c("axial", 2, 3, 64, 5, 7, 128),
    # height pass fused, width pass generic (L > 128): not lean
    "w_over_128_keys": _c("axial", 1, 2, 256, 16, 132),
    # L < 8: generic height pass
    "h_under_8_keys": _c("axial", 1, 2, 256, 4, 16),
    # 672 tiles > 640 with L != 64: 64-row tiles NOT merged -- and merged under merge_qkv_any
    "over_640_tiles": _c("axial", 1, 4, 256, 96, 112),
    "over_640_tiles_any": _c("axial", 1, 4, 256, 96, 112, 1024, [("merge_qkv_any", 1)]),
    # GELU: the FFN does not ride; stand-alone fused GELU kernel
    "gelu": _c("axial", 1, 4, 256, 64, 64, activation="gelu"),
    # 128-row (wide) FFN tiles just pay / just do not
    "ffn_wide_pays": _c("ffn", 1, 1, 256, 16448, 1),
    "ffn_wide_does_not": _c("ffn", 1, 1, 256, 16384, 1),
    # frames of 272 keys: the long spatial kernel
    "full_272_keys": _c("full", 1, 2, 256, 17, 16),
    # frames of 576 keys: three key chunks of the long spatial kernel (256 + 256 + 64)
    "full_576_keys": _c("full", 1, 2, 256, 24, 24),
    # strided frames: a 16 x 16 level inside a 336-row token buffer
    "in_place_level": _c("axial", 1, 2, 256, 16, 16, sine=True, in_place=336),
    # sine positions materialised (C != 256) / generated in the kernel
    "sine_materialised": _c("axial", 1, 2, 128, 16, 12, sine=True),
    "sine_in_kernel": _c("axial", 1, 2, 256, 16, 12, sine=True),
    # cross-clip layer: the post-norm rides in the trajectory kernel / is its own launch
    "cc_ln_in_kernel": _c("cc", 1, 3, 256, 16, 1),
    "cc_ln_own_launch": _c("cc", 1, 13, 256, 16, 1),
}
# every option the planner reads, at the base shape
CASES.update({f"base_{k}": _c("axial", *BASE, 1024, [(k, 1)]) for k in ("generic_only", "no_attn_fusion", "no_ffn_fusion", "no_merge_qkv")})
CASES.update({f"base_plan_force_{b}": _c("axial", *BASE, 1024, [("plan_force", b)]) for b in (1, 2, 4, 8, 16, 32)})

# stage names per case, as recorded from the library before the refactor
STAGES = {
    "mq2_ffn_rides": ['begin', 'h.qkv+traj', 'w.qkv+traj+ffn'],
    "mq2_ffn_rides_f16_out": ['begin', 'h.qkv+traj', 'w.qkv+traj+ffn'],
    "mq1_frames_32_48": ['begin', 'h.qkv+traj', 'w.qkv+traj+ffn'],
    "first_on_64_rows": ['begin', 'h.qkv+traj', 'w.qkv+traj+ffn'],
    "last_on_few_rows": ['begin', 'h.qkv+traj', 'w.qkv+traj', 'norm1+ffn+norm2'],
    "last_on_16_rows": ['begin', 'h.qkv_proj', 'h.traj_fused', 'w.qkv_proj', 'w.traj_fused', 'norm1+ffn+norm2'],
    "rows16_merged": ['begin', 'h.qkv+traj', 'w.qkv+traj', 'norm1+ffn+norm2'],
    "rows16_two_launches": ['begin', 'h.qkv_proj', 'h.traj_fused', 'w.qkv_proj', 'w.traj_fused', 'norm1+ffn+norm2'],
    "rows16_ragged": ['begin', 'h.qkv_proj', 'h.traj_fused', 'w.qkv_proj', 'w.traj_fused', 'norm1+ffn+norm2'],
    "rows32_merged_split2": ['begin', 'h.qkv+traj', 'w.qkv+traj', 'norm1+ffn+norm2'],
    "rows32_two_launches": ['begin', 'h.qkv_proj', 'h.traj_fused', 'w.qkv_proj', 'w.traj_fused', 'norm1+ffn+norm2'],
    "t9_rows16": ['begin', 'h.qkv_proj', 'h.traj_fused', 'w.qkv_proj', 'w.traj_fused', 'norm1+ffn+norm2'],
    "maps_temporal_fused": ['begin', 'h.qkv_proj', 'h.spatial_attn', 'h.temporal_fused', 'w.qkv_proj', 'w.spatial_attn', 'w.temporal_fused', 'norm1+ffn+norm2'],
    "t13_reassoc": ['begin', 'h.qkv_proj', 'h.spatial_attn', 'h.proj_q', 'h.proj_kv', 'h.temporal_attn', 'h.proj', 'w.qkv_proj', 'w.spatial_attn', 'w.proj_q', 'w.proj_kv', 'w.temporal_attn', 'w.proj', 'norm1+ffn+norm2'],
    "t13_no_reassoc": ['begin', 'h.qkv_proj', 'h.spatial_attn', 'h.proj_q', 'h.proj_kv', 'h.temporal_attn', 'h.proj', 'w.qkv_proj', 'w.spatial_attn', 'w.proj_q', 'w.proj_kv', 'w.temporal_attn', 'w.proj', 'norm1+ffn+norm2'],
    "generic_c64": ['begin', 'h.qkv_proj', 'h.spatial_attn', 'h.proj_q', 'h.proj_kv', 'h.temporal_attn', 'h.proj', 'w.qkv_proj', 'w.spatial_attn', 'w.proj_q', 'w.proj_kv', 'w.temporal_attn', 'w.proj', 'norm1', 'ffn.linear1', 'ffn.linear2', 'norm2'],
    "w_over_128_keys": ['begin', 'h.qkv+traj', 'w.qkv_proj', 'w.spatial_attn', 'w.temporal_fused', 'norm1+ffn+norm2'],
    "h_under_8_keys": ['begin', 'h.qkv_proj', 'h.spatial_attn', 'h.temporal_fused', 'w.qkv+traj', 'norm1+ffn+norm2'],
    "over_640_tiles": ['begin', 'h.qkv_proj', 'h.traj_fused', 'w.qkv_proj', 'w.traj_fused+ffn'],
    "over_640_tiles_any": ['begin', 'h.qkv+traj', 'w.qkv_proj', 'w.traj_fused+ffn'],
    "gelu": ['begin', 'h.qkv+traj', 'w.qkv+traj', 'norm1+ffn+norm2'],
    "ffn_wide_pays": ['norm1+ffn+norm2'],
    "ffn_wide_does_not": ['norm1+ffn+norm2'],
    "full_272_keys": ['begin', 'qkv_proj', 'spatial_attn', 'temporal_fused', 'norm1+ffn+norm2'],
    "full_576_keys": ['begin', 'qkv_proj', 'spatial_attn', 'temporal_fused', 'norm1+ffn+norm2'],
    "in_place_level": ['begin', 'h.qkv+traj', 'w.qkv+traj', 'norm1+ffn+norm2'],
    "sine_materialised": ['begin', 'pos3d', 'h.qkv_proj', 'h.spatial_attn', 'h.proj_q', 'h.proj_kv', 'h.temporal_attn', 'h.proj', 'w.qkv_proj', 'w.spatial_attn', 'w.proj_q', 'w.proj_kv', 'w.temporal_attn', 'w.proj', 'norm1', 'ffn.linear1', 'ffn.linear2', 'norm2'],
    "sine_in_kernel": ['begin', 'h.qkv+traj', 'w.qkv+traj', 'norm1+ffn+norm2'],
    "cc_ln_in_kernel": ['begin', 'qkv+traj', 'cc.aspp', 'cc.aspp_post', 'cc.embeddings', 'cc.class_head', 'cc.mask_einsum'],
    "cc_ln_own_launch": ['begin', 'qkv_proj', 'spatial_attn', 'proj_q', 'proj_kv', 'temporal_attn', 'proj', 'cc.norm', 'cc.aspp', 'cc.aspp_post', 'cc.embeddings', 'cc.class_head', 'cc.mask_einsum'],
    "base_generic_only": ['begin', 'h.qkv_proj', 'h.spatial_attn', 'h.proj_q', 'h.proj_kv', 'h.temporal_attn', 'h.proj', 'w.qkv_proj', 'w.spatial_attn', 'w.proj_q', 'w.proj_kv', 'w.temporal_attn', 'w.proj', 'norm1', 'ffn.linear1', 'ffn.linear2', 'norm2'],
    "base_no_attn_fusion": ['begin', 'h.qkv_proj', 'h.spatial_attn', 'h.temporal_fused', 'w.qkv_proj', 'w.spatial_attn', 'w.temporal_fused', 'norm1+ffn+norm2'],
    "base_no_ffn_fusion": ['begin', 'h.qkv+traj', 'w.qkv+traj', 'norm1+ffn+norm2'],
    "base_no_merge_qkv": ['begin', 'h.qkv_proj', 'h.traj_fused', 'w.qkv_proj', 'w.traj_fused+ffn'],
    "base_plan_force_1": ['begin', 'h.qkv+traj', 'w.qkv+traj+ffn'],
    "base_plan_force_2": ['begin', 'h.qkv+traj', 'w.qkv+traj+ffn'],
    "base_plan_force_4": ['begin', 'h.qkv+traj', 'w.qkv+traj+ffn'],
    "base_plan_force_8": ['begin', 'h.qkv+traj', 'w.qkv+traj+ffn'],
    "base_plan_force_16": ['begin', 'h.qkv+traj', 'w.qkv+traj+ffn'],
    "base_plan_force_32": ['begin', 'h.qkv+traj', 'w.qkv+traj+ffn'],
}

CC_LAYERS, CC_CLASSES, CC_PIXELS = 1, 11, (1, 5, 7)      # the cross-clip module around the layer: (V, H, W) of the pixel features


def _weights(c, seed=SEED):
    if c.kind == "cc":
        return orc.random_weights(orc.cc_module_param_shapes(CC_LAYERS, CC_CLASSES), seed)
    shapes = orc.axial_layer_param_shapes(c.C, c.F)
    if c.kind == "full":
        shapes = {k.replace("height_attn", "temporal_attn"): v for k, v in shapes.items() if "width_attn" not in k}
    return orc.random_weights(shapes, seed)


def _inputs(c):
    """CPU fp32 inputs: (src, pos) of a clip, (x,) of the FFN, (clip_query, pixel_features) of the cross-clip module.  `pos` of a
    sine case is made on the device by the runner."""
    g = torch.Generator().manual_seed(SEED + 1)
    if c.kind == "ffn":
        return (torch.randn(c.H, c.C, generator=g) * 2 + 0.3,)
    if c.kind == "cc":
        V, H, W = CC_PIXELS
        return (torch.randn(c.B, c.H, c.T, 256, generator=g),
                torch.nn.functional.normalize(torch.randn(c.B, 128, c.T * V, H, W, generator=g), dim=1))
    return orc.synthetic_clip(c.B, c.T, c.C, c.H, c.W, SEED)


def _tokens(c, src):
    """the token buffer of an in-place case: the level's rows at [start, start + H W) of every frame, random rows around them"""
    S, start = c.extras["in_place"], 40
    buf = torch.randn(c.B * c.T, S, c.C, generator=torch.Generator().manual_seed(SEED + 2))
    buf[:, start:start + c.H * c.W] = src
    return buf, start


def _stage_names():
    from axial_vs_amd import _lib
    L = _lib.lib()
    return [L.axvs_profile_stage_name(i).decode() for i in range(L.axvs_profile_stage_count())]


_modules = {}


def _module(c, weights=None):
    """the case's module on the device, built once per (kind, sizes, activation); weights: a module of its own with these parameters
    in place of _weights(c), not kept"""
    import axial_vs_amd as ax
    key = (c.kind, c.C, c.F, c.extras.get("activation", "relu"))
    if weights is not None or key not in _modules:
        w = _weights(c) if weights is None else dict(weights)
        if c.kind == "cc":
            V = CC_PIXELS[0]
            mod = ax.CrossClipTrackingModule(num_layers=CC_LAYERS, num_classes=CC_CLASSES, attn_drop=0.0, aspp_drop=0.0, kernel_sizes=[3, 3, 3],
                                             atrous_rates=[1, 2, 3], norm_fn="ln", num_clip_frames=V)
            sd = mod.state_dict()
            sd.update(w)
            w = sd
        elif c.kind == "full":
            mod = ax.TemporalTrajectoryAttentionLayer(c.C, c.F, n_heads=8)
        else:
            mod = ax.TemporalAxialTrajectoryAttentionLayer(c.C, c.F, n_heads=8, activation=key[3])
        mod.load_state_dict(w, strict=True)
        if weights is not None:
            return mod.eval().cuda()
        _modules[key] = mod.eval().cuda()
    return _modules[key]


def run(name, weights=None):
    """One eval forward of the case on the device -> ({label: tensor}, stage names).  "out" is what `reference` answers for.
    weights: the parameters to load in place of _weights(c) (tests/infer_regime_cases.py)."""
    import axial_vs_amd as ax
    from axial_vs_amd import _lib
    c = CASES[name]
    L = _lib.lib()
    mod = _module(c, weights)
    ins = [x.cuda() for x in _inputs(c)]
    for k, v in c.options:
        _lib.check(L.axvs_set_option(k.encode(), v), "axvs_set_option")
    try:
        if c.kind == "ffn":
            M, x = c.H, ins[0]
            ws = torch.empty(L.axvs_ffn_workspace_bytes(M, c.C, c.F), dtype=torch.uint8, device="cuda")
            out = torch.empty_like(x)
            _lib.check(L.axvs_ffn_fwd(x.data_ptr(), out.data_ptr(), mod._pack().data_ptr(), M, c.C, 8, c.F, 0, ws.data_ptr(), ws.numel(),
                                      torch.cuda.current_stream().cuda_stream), "axvs_ffn_fwd")
            outs = {"out": out}
        elif c.kind == "cc":
            res = mod(*ins)
            outs = {"out": res["pred_masks"], "pred_logits": res["pred_logits"]}
        elif c.kind == "full":
            outs = {"out": mod(*ins)[0]}
        else:
            src, pos = ins
            if c.extras.get("sine"):
                pos = ax.PositionEmbeddingSine3D(c.C // 2, normalize=True).channels_last(c.B, c.T, c.H, c.W, "cuda")
            if "in_place" in c.extras:
                buf, start = _tokens(c, src.cpu())
                buf = buf.cuda()
                assert mod.can_run_in_place(pos)
                mod.forward_level_in_place(buf, start, pos)
                outs = {"out": buf}
            else:
                mod.out_dtype, mod.return_attn = c.extras.get("out_dtype"), bool(c.extras.get("return_attn"))
                try:
                    out, ha, wa = mod(src, pos)
                finally:
                    mod.out_dtype, mod.return_attn = None, False
                outs = {"out": out}
                if ha is not None:
                    outs.update(h_attn=ha, w_attn=wa)
        names = _stage_names()
        torch.cuda.synchronize()
    finally:
        for k, _ in c.options:
            L.axvs_set_option(k.encode(), 0)
    return outs, names


_refs = {}


def reference(name):
    """float64 oracle for the case's "out" (CPU).  Computed once per distinct computation and shared: leave it unchanged."""
    c = CASES[name]
    key = (c.kind, c.B, c.T, c.C, c.H, c.W, c.F, c.extras.get("activation", "relu"), bool(c.extras.get("sine")), c.extras.get("in_place"))
    if key not in _refs:
        w = {k: v.double() for k, v in _weights(c).items()}
        ins = [x.double() for x in _inputs(c)]
        if c.kind == "ffn":
            y = orc._layer_norm(ins[0], w, "norm1")
            ref = orc._layer_norm(y + orc._linear(torch.relu(orc._linear(y, w, "linear1")), w, "linear2"), w, "norm2")
        elif c.kind == "cc":
            ref = orc.cross_clip_module(ins[0], ins[1], w, CC_LAYERS, CC_PIXELS[0])["pred_masks"]
        elif c.kind == "full":
            ref = orc.trajectory_layer(ins[0], ins[1], w, 8)
        else:
            src, pos = ins
            if c.extras.get("sine"):
                import axial_vs_amd as ax
                pos = ax.PositionEmbeddingSine3D(c.C // 2, normalize=True).channels_last(c.B, c.T, c.H, c.W, "cuda").cpu().double()
            ref = orc.axial_layer(src, pos, w, 8, want_attn=False, activation=c.extras.get("activation", "relu"))[0]
            if "in_place" in c.extras:
                buf, start = _tokens(c, src.float())
                buf = buf.double()
                buf[:, start:start + c.H * c.W] = ref
                ref = buf
        _refs[key] = ref
    return _refs[key]
