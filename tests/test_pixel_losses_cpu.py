"""CPU: the float64 restatement of the sampled pixel losses against the reference's stored fp32 values and sample sets, the noise
draw, and the host surface of axial_vs_amd.sampled_pixel_losses / MaXTronWCSetCriterion with all four losses (no GPU needed)."""
import ctypes
import inspect
import json
import os
import re

import pytest
import torch

import __graft_entry__ as ge
import pixel_loss_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FOUR = ["labels", "masks", "pixels", "aux_semantic"]


@pytest.fixture(scope="module", autouse=True)
def built():
    ge.build()


@pytest.mark.parametrize("name", list(pc.CASES))
def test_restatement_selects_the_reference_sets_and_agrees_within_the_fp32_bound(name):
    """the float64 sample sets ARE the reference's fp32 ones (the screen's promise), every row passes the screen as stored, and the
    reference's fp32 losses and gradients lie within the format-derived bound of the restatement"""
    fx = pc.fixture(name)
    case = pc.CASES[name]
    m = fx.meta
    assert (m["N"], tuple(m["M"]), m["K"], m["T"], m["H"], m["W"], m["L"], m["share"], m["kind"], m["C"], m["kp"], m["ks"], m["semkind"]) == case
    assert json.load(open(pc.SEEDS))[name] == {"seed": m["seed"], "noise_seed": m["noise_seed"]}
    for r, per in enumerate(fx.sets64()):
        for b, (idx, key, void, gap) in enumerate(per):
            assert torch.equal(idx, fx.ref_samples[r][b]), (r, b)
            assert gap > 0.0
    assert 0.0 <= m["screen_used"] < 1.0
    el, eg = fx.reference_errors()
    bound = pc.fp32_bound(max(fx.C, fx.K), max(fx.kp, fx.ks))
    print(f"{name}: reference fp32 error  losses {el:.3e}  gradients {eg:.3e}  bound {bound:.3e}")
    assert el < bound and eg < bound
    losses, _, _ = fx.restated()
    assert list(losses) == fx.keys == pc.loss_keys(fx.L)


def test_cases_have_the_properties_they_are_there_for():
    fx = pc.fixture("g25_pixel_losses_M0")
    void = fx.sets64()[0][1][2]
    assert bool(void.all()) and fx.kp == fx.P                                   # the second video is all void and every pixel is taken
    losses, df, _ = fx.restated()
    assert float(df[0][1].abs().max()) == 0.0 and float(df[0][0].abs().max()) > 0.0     # ... so its insdis term is exactly 0
    fx = pc.fixture("g25_pixel_losses_semignore")
    assert all(bool((t["semantic_masks"] == -1).all()) for t in fx.targets)
    assert fx.ref_losses["loss_aux_semantic"] == 0.0 and float(fx.restated()[0]["loss_aux_semantic"]) == 0.0
    fx = pc.fixture("g25_pixel_losses_MgtN")
    assert fx.meta["M"][0] > fx.N and len(fx.pairs[0][0][0]) == fx.N
    fx = pc.fixture("g25_pixel_losses_float")
    t = fx.targets[0]["masks"].flatten(1)
    assert t.dtype == torch.float32 and bool(((t > 0).sum(0) > 1).any()) and bool(((t > 0) & (t < 1)).any())      # overlapping, non-binary
    fx = pc.fixture("g25_pixel_losses_k65_own")
    assert not fx.share and len(fx.pairs) == fx.L == 2 and fx.meta["M"] == [4, 2]
    for name in ("g25_pixel_losses_k1", "g25_pixel_losses_k63", "g25_pixel_losses_k64"):     # void pixels exist and none is sampled
        fx = pc.fixture(name)
        for per in fx.sets64():
            for idx, key, void, gap in per:
                assert bool(void.any()) and not bool(void[idx].any())
    # the unscreened case: fewer non-void pixels than k
    case = pc.UNSCREENED_CASES["sparse_k40"]
    _, targets = pc.make_case(case, 0)
    assert int(targets[0]["masks"].flatten(1).any(0).sum()) == 10 < case[10]


@pytest.mark.parametrize("name", ["g25_pixel_losses_k63", "g25_pixel_losses_k65_own", "g25_pixel_losses_P1100"])
def test_draw_sampling_noise_consumes_the_generator_like_the_reference(name):
    """the stored u is what the reference drew under the stored seed; draw_sampling_noise reproduces it, from the default generator and
    from an explicit one, and leaves the generator where the reference leaves it"""
    import axial_vs_amd as ax
    fx = pc.fixture(name)
    torch.manual_seed(fx.meta["noise_seed"])
    up, us = ax.draw_sampling_noise(fx.L, fx.B, fx.P, True, True, "cpu")
    after = torch.rand(3)
    assert torch.equal(up, fx.u_pix) and torch.equal(us, fx.u_sem)
    torch.manual_seed(fx.meta["noise_seed"])
    stream = [torch.rand((fx.B, fx.P)) for _ in range(fx.L + 1)]                  # the reference's calls: (B, P) each, in forward's order
    assert torch.equal(torch.rand(3), after)
    assert torch.equal(stream[0], up[0]) and torch.equal(stream[1], us) and all(torch.equal(stream[1 + l], up[l]) for l in range(1, fx.L))
    g = torch.Generator().manual_seed(fx.meta["noise_seed"])
    up2, us2 = ax.draw_sampling_noise(fx.L, fx.B, fx.P, True, True, "cpu", generator=g)
    assert torch.equal(up2, up) and torch.equal(us2, us)
    # one loss only: only its draws
    torch.manual_seed(fx.meta["noise_seed"])
    up3, us3 = ax.draw_sampling_noise(fx.L, fx.B, fx.P, True, False, "cpu")
    assert us3 is None and torch.equal(up3[0], stream[0]) and (fx.L == 1 or torch.equal(up3[1], stream[1]))
    torch.manual_seed(fx.meta["noise_seed"])
    up4, us4 = ax.draw_sampling_noise(fx.L, fx.B, fx.P, False, True, "cpu")
    assert up4 is None and torch.equal(us4, stream[0])


def _declared_arg_count(name):
    text = open(os.path.join(ROOT, "include", "axvs.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    args = re.search(r"\b" + name + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
    return len([a for a in args.split(",") if a.strip()])


def test_entry_points_are_bound_and_refuse_bad_arguments_before_any_device_work():
    from axial_vs_amd import _lib
    L = _lib.lib()
    names = ("axvs_pixel_sample", "axvs_pixel_insdis_saved_bytes", "axvs_pixel_insdis_workspace_bytes", "axvs_pixel_insdis_fwd",
             "axvs_pixel_insdis_bwd", "axvs_pixel_semantic_saved_bytes", "axvs_pixel_semantic_fwd", "axvs_pixel_semantic_bwd")
    for name in names:
        assert hasattr(L, name)
        assert len(_lib.SIGNATURES[name][1]) == _declared_arg_count(name), name
    sv, ws, ssv = L.axvs_pixel_insdis_saved_bytes, L.axvs_pixel_insdis_workspace_bytes, L.axvs_pixel_semantic_saved_bytes
    assert 0 < sv(7, 2, 4096) < 7 * 2 * 4096 * 4 * 4                        # O(L B k): nothing like a [k, k] matrix
    assert ws(7, 2, 128, 32, 4096) == 7 * 2 * 4096 * (128 + 32) * 4
    assert sv(1, 1, 0) > 0 and ws(1, 1, 4, 0, 0) > 0 and ssv(1, 0) > 0
    for bad, word in ((lambda: sv(17, 1, 8), b"L=17"), (lambda: sv(1, 65, 8), b"B=65"), (lambda: sv(1, 1, 8193), b"k=8193"),
                      (lambda: ws(1, 1, 6, 0, 8), b"C=6"), (lambda: ws(1, 1, 260, 0, 8), b"C=260"), (lambda: ws(1, 1, 8, 513, 8), b"kmax=513"),
                      (lambda: ws(1, 1, 8, 0, 8193), b"k=8193"), (lambda: ssv(1, 8193), b"k=8193"), (lambda: ssv(65, 1), b"B=65")):
        assert bad() == 0 and word in L.axvs_last_error(), word
    one = (ctypes.c_void_p * 1)(16)
    m1 = (ctypes.c_int * 1)(3)

    def fwd(feat=one, tgt=16, tdt=_lib.AXVS_U8, m=m1, cols=16, kmax=3, Ln=1, B=1, N=8, Cf=8, P=120, idx=16, k=10, kstride=10, losses=16, saved=16,
            wsp=16, wsb=1 << 30):
        return L.axvs_pixel_insdis_fwd(feat, tgt, tdt, m, cols, kmax, 1, Ln, B, N, Cf, P, idx, k, kstride, losses, saved, wsp, wsb, None)

    for kw in (dict(feat=None), dict(tgt=None), dict(m=None), dict(cols=None), dict(idx=None), dict(losses=None), dict(saved=None), dict(wsp=None),
               dict(feat=(ctypes.c_void_p * 1)(None))):
        assert fwd(**kw) == -1 and b"null" in L.axvs_last_error(), kw
    for kw, word in ((dict(Ln=17), b"L=17"), (dict(B=65), b"B=65"), (dict(N=513), b"N=513"), (dict(Cf=10), b"C=10"), (dict(Cf=260), b"C=260"),
                     (dict(P=(1 << 20) + 1), b"P=1048577"), (dict(k=8193, kstride=8193, P=10000), b"k=8193"), (dict(k=121, kstride=121), b"k=121"),
                     (dict(kstride=9), b"kstride=9"), (dict(kmax=9), b"kmax=9"), (dict(tdt=0), b"dtype 0"),
                     (dict(m=(ctypes.c_int * 1)(513)), b"513")):
        assert fwd(**kw) == -1 and word in L.axvs_last_error(), (kw, L.axvs_last_error())
    assert fwd(wsb=16) == -2 and b"workspace too small" in L.axvs_last_error()
    assert L.axvs_pixel_insdis_bwd(None, one, 16, _lib.AXVS_U8, m1, 16, 3, 1, 1, 1, 8, 8, 120, 16, 10, 10, 16, one, 16, 1 << 30, None) == -1
    assert L.axvs_pixel_insdis_bwd(16, one, 16, _lib.AXVS_U8, m1, 16, 3, 1, 1, 1, 8, 8, 120, 16, 10, 10, 16, one, 16, 16, None) == -2
    # k > P is refused as torch.topk refuses it
    assert L.axvs_pixel_semantic_fwd(16, 16, 16, 121, 121, 1, 5, 120, 5, 16, 16, None) == -1 and b"out of range" in L.axvs_last_error()
    assert L.axvs_pixel_semantic_fwd(16, 16, 16, 10, 10, 1, 257, 120, 5, 16, 16, None) == -1 and b"257" in L.axvs_last_error()
    assert L.axvs_pixel_semantic_bwd(16, 16, 16, 16, 10, 10, 1, 5, 120, 5, 16, None, None) == -1 and b"null" in L.axvs_last_error()
    u = (ctypes.c_void_p * 1)(16)
    i1, f1 = (ctypes.c_int * 1), (ctypes.c_float * 1)
    assert L.axvs_pixel_sample(16, _lib.AXVS_U8, m1, 16, 3, 1, 1, 8, 120, u, i1(0), f1(1.5), i1(121), 1, 16, 16, 16, 121, None) == -1
    assert b"k=121" in L.axvs_last_error()
    assert L.axvs_pixel_sample(16, _lib.AXVS_U8, m1, 16, 3, 1, 1, 8, 120, u, i1(1), f1(1.5), i1(10), 1, 16, 16, 16, 10, None) == -1
    assert b"row_matching" in L.axvs_last_error()
    assert L.axvs_pixel_sample(16, _lib.AXVS_U8, m1, 16, 3, 1, 1, 8, 120, u, i1(0), f1(1.5), i1(10), 18, 16, 16, 16, 10, None) == -1
    assert b"R=18" in L.axvs_last_error()


def test_cpu_tensors_and_bounds_raise():
    import axial_vs_amd as ax
    fx = pc.fixture("g25_pixel_losses_k1")
    with pytest.raises(RuntimeError, match="GPU"):
        ax.sampled_pixel_losses(fx.outputs(), fx.targets, fx.K, noise=(fx.u_pix, fx.u_sem))
    crit = ax.MaXTronWCSetCriterion(fx.K, ax.VideoHungarianMatcher(), {}, 0.1, FOUR, True, process_semantic=True)
    with pytest.raises(RuntimeError, match="GPU"):
        crit(fx.outputs(), fx.targets)
    with pytest.raises(ValueError, match="labels"):
        ax.sampled_pixel_losses(fx.outputs(), fx.targets, fx.K, losses=("labels",))


def test_the_within_clip_constructor_accepts_the_four_losses_and_mirrors_the_attributes():
    import axial_vs_amd as ax
    m, wd = ax.VideoHungarianMatcher(), {"loss_ce": 3.0}
    c = ax.MaXTronWCSetCriterion(124, m, wd, 0.1, FOUR, True, process_semantic=True, pixel_insdis_temperature=1.8, aux_semantic_temperature=2.4)
    assert (c.num_classes, c.matcher, c.weight_dict, c.eos_coef, c.losses, c.share_final_matching) == (124, m, wd, 0.1, FOUR, True)
    assert (c.process_semantic, c.pixel_insdis_temperature, c.pixel_insdis_sample_k, c.aux_semantic_temperature, c.aux_semantic_sample_k,
            c.masking_void_pixel) == (True, 1.8, 4096, 2.4, 4096, True)
    c = ax.MaXTronWCSetCriterion(19, m, wd, 0.1, ["pixels"], False, pixel_insdis_sample_k=0, aux_semantic_sample_k=7, masking_void_pixel=False)
    assert (c.losses, c.pixel_insdis_sample_k, c.aux_semantic_sample_k, c.masking_void_pixel, c.share_final_matching) == (["pixels"], 0, 7, False, False)
    assert list(inspect.signature(ax.MaXTronWCSetCriterion.forward).parameters) == ["self", "outputs", "targets"]
    with pytest.raises(NotImplementedError, match="aux_contrast"):
        ax.MaXTronWCSetCriterion(19, m, wd, 0.1, ["labels", "aux_contrast"], True)
    for loss in ("pixels", "aux_semantic"):                                   # the cross-clip criterion keeps refusing them
        with pytest.raises(NotImplementedError, match="Gumbel"):
            ax.MaXTronCCSetCriterion(19, m, wd, 0.1, ["labels", "masks", loss], True)
    assert "draw_sampling_noise" in ax.__all__ and "sampled_pixel_losses" in ax.__all__
