"""GPU: the regular-tile instantiation of the merged q/k/v + trajectory kernels (TrajPlan::reg, temporal_fused_kernel<..., REG>) and
the compile-time output forms of the row tails against the shape-generic instantiation -- same bits -- and against the float64 oracle.

A pass runs the regular-tile instantiation when its frames are whole, unpadded 64-key frames (a 64-row tile is one frame), the row
offsets fit 32 bits and the rows leave as fp32; `plan_force` 128 forces the generic instantiation, `axvs_plan_regular_tiles()` says
which one the last height (bit 0) / width (bit 1) pass ran."""
import pytest
import torch

import __graft_entry__ as ge
import axvs_oracle as orc
from golden_util import ELEM_RTOL, elem_check, rel_err      # ELEM_RTOL = 1e-3: the parity bar, as max-norm and per element

pytestmark = pytest.mark.gpu

FORCE_GENERIC = 128      # plan_force bit: never the regular-tile instantiation


@pytest.fixture(scope="module", autouse=True)
def built():
    ge.build()
    assert torch.cuda.is_available()


def _lib():
    from axial_vs_amd import _lib as L
    return L


def _both(run):
    """run() under the planner's own choice and with the generic instantiation forced: (out, passes), (out, passes)"""
    L = _lib()
    own = run().clone()
    own_passes = L.lib().axvs_plan_regular_tiles()
    L.check(L.lib().axvs_set_option(b"plan_force", FORCE_GENERIC), "axvs_set_option")
    try:
        gen = run().clone()
        gen_passes = L.lib().axvs_plan_regular_tiles()
    finally:
        L.lib().axvs_set_option(b"plan_force", 0)
    return (own, own_passes), (gen, gen_passes)


def _stage_names():
    L = _lib().lib()
    return [L.axvs_profile_stage_name(i).decode() for i in range(L.axvs_profile_stage_count())]


def _layer(C, F, seed):
    import axial_vs_amd as ax
    w = orc.random_weights(orc.axial_layer_param_shapes(C, F), seed)
    layer = ax.TemporalAxialTrajectoryAttentionLayer(C, F, n_heads=8).eval()
    layer.load_state_dict(w, strict=True)
    return layer.cuda(), w


def _check_oracle(out, ref, what):
    e = rel_err(out.cpu(), ref)
    print(f"{what}: max/max {e:.2e}")
    elem_check(out.cpu(), ref, what)
    assert e < ELEM_RTOL


# (shape, passes that run the regular-tile instantiation: bit 0 height, bit 1 width)
SHAPES = [((1, 2, 256, 64, 64), 3),      # both passes regular, a tile is a frame (MQ = 2), the FFN rides in the width pass
          ((2, 2, 256, 64, 64), 3),      # batch > 1: the tile -> (batch, off-axis coordinate) decomposition
          ((1, 4, 256, 64, 20), 1),      # height pass regular; width pass: frames of 20 keys padded to 32 -> generic
          ((1, 2, 256, 49, 85), 0)]      # ragged on both axes (49 -> 64, 85 -> 96): generic on both passes


@pytest.mark.parametrize("shape,passes", SHAPES)
def test_regular_tiles_are_bit_identical_to_the_generic_instantiation(shape, passes):
    B, T, C, H, W = shape
    F = 1024
    layer, w = _layer(C, F, 91)
    src, pos = orc.synthetic_clip(B, T, C, H, W, 91)
    ref, _, _ = orc.axial_layer(src.double(), pos.double(), w, 8, want_attn=False)
    s, p = src.cuda(), pos.cuda()
    (own, own_passes), (gen, gen_passes) = _both(lambda: layer(s, p)[0])
    names = _stage_names()
    print(f"{shape}: {names[1:]}, regular passes {own_passes} (forced generic: {gen_passes})")
    assert own_passes == passes and gen_passes == 0
    if passes & 1:
        assert "h.qkv+traj" in names      # the regular-tile instantiation exists for merged launches only
    if passes & 2:
        assert "w.qkv+traj+ffn" in names
    assert torch.equal(own, gen)
    _check_oracle(own, ref, f"regular tiles {shape}")


def test_generated_positions_and_strided_frames_on_regular_tiles():
    """The level-in-place call (frames a stride apart in a token buffer, positions generated in the kernel with a level embedding):
    the regular-tile instantiation evaluates the frame term of the sine positions once per wave and addresses rows as the tile's
    offset plus l * sL -- same bits as the generic instantiation, in place and out of place."""
    import axial_vs_amd as ax
    B, T, C, H, W, F, S = 1, 2, 256, 64, 64, 1024, 64 * 64 + 336
    layer, w = _layer(C, F, 93)
    g = torch.Generator().manual_seed(5)
    level = torch.randn(C, generator=g).cuda()
    pos = ax.PositionEmbeddingSine3D(C // 2, normalize=True).channels_last_with_level(B, T, H, W, level)
    tokens = torch.randn(B * T, S, C, generator=g).cuda()
    start = 200
    lvl = tokens[:, start:start + H * W].contiguous()
    ref, _, _ = orc.axial_layer(lvl.cpu().double(), pos.cpu().double(), w, 8, want_attn=False)
    assert layer.can_run_in_place(pos)

    def in_place():
        buf = tokens.clone()
        layer.forward_level_in_place(buf, start, pos)
        return buf

    (own, own_passes), (gen, gen_passes) = _both(in_place)
    assert own_passes == 3 and gen_passes == 0
    assert torch.equal(own, gen)
    assert torch.equal(own[:, :start], tokens[:, :start]) and torch.equal(own[:, start + H * W:], tokens[:, start + H * W:])
    (cown, cown_passes), (cgen, _) = _both(lambda: layer(lvl, pos)[0])
    assert cown_passes == 3
    assert torch.equal(cown, cgen) and torch.equal(own[:, start:start + H * W], cown)
    _check_oracle(cown, ref, "generated positions, level in place")


def test_16_bit_output_map_keeps_the_width_pass_on_the_generic_instantiation():
    """out_dtype = float16: the rows of the FFN-carrying kernel leave as a 16-bit map, a form the regular-tile instantiation is not
    built for -- the width pass stays generic (the height pass does not), and the map is the fp32 output rounded once."""
    B, T, C, H, W, F = 1, 2, 256, 64, 64, 1024
    layer, w = _layer(C, F, 91)
    src, pos = orc.synthetic_clip(B, T, C, H, W, 91)
    ref, _, _ = orc.axial_layer(src.double(), pos.double(), w, 8, want_attn=False)
    s, p = src.cuda(), pos.cuda()
    full = layer(s, p)[0].clone()
    layer.out_dtype = torch.float16
    try:
        (own, own_passes), (gen, gen_passes) = _both(lambda: layer(s, p)[0])
    finally:
        layer.out_dtype = None
    assert own.dtype == torch.float16 and own_passes == 1 and gen_passes == 0
    assert torch.equal(own, gen) and torch.equal(own, full.half())
    _check_oracle(full, ref, "fp32 map behind the f16 one")


def test_post_norm_rows_of_the_cross_clip_layers():
    """The post-norm row epilogue (LayerNorm(x + attn(x)) of the cross-clip layers, 16-row tiles): picked once per tail, rows in
    straight-line code.  Smallest fixture shape of the cross-clip module (16 queries, 3 clips) against the float64 oracle; these
    passes are never regular tiles, so forcing the generic instantiation changes nothing."""
    import axial_vs_amd as ax
    B, Q, Tc, nl, K, V, H, W = 1, 16, 3, 2, 11, 2, 8, 8
    w = orc.random_weights(orc.cc_module_param_shapes(nl, K), 61)
    g = torch.Generator().manual_seed(62)
    cq = torch.randn(B, Q, Tc, 256, generator=g)
    pf = torch.nn.functional.normalize(torch.randn(B, 128, Tc * V, H, W, generator=g), dim=1)
    ref = orc.cross_clip_module(cq.double(), pf.double(), {k: v.double() for k, v in w.items()}, nl, V)
    mod = ax.CrossClipTrackingModule(num_layers=nl, num_classes=K, attn_drop=0.0, aspp_drop=0.0, kernel_sizes=[3, 3, 3], atrous_rates=[1, 2, 3],
                                     norm_fn="ln", num_clip_frames=V).eval()
    sd = mod.state_dict()
    sd.update(w)
    mod.load_state_dict(sd, strict=True)
    mod = mod.cuda()
    c, f = cq.cuda(), pf.cuda()
    (own, own_passes), (gen, gen_passes) = _both(lambda: mod(c, f)["pred_masks"])
    assert own_passes == 0 and gen_passes == 0
    assert torch.equal(own, gen)
    _check_oracle(own, ref["pred_masks"], "cross-clip post-norm")
    assert rel_err(mod(c, f)["pred_logits"], ref["pred_logits"]) < ELEM_RTOL
