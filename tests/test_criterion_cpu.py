"""CPU: the set criterion's float64 restatement against the reference's stored fp32 values, and the host surface of
axial_vs_amd.MaXTronCCSetCriterion / MaXTronWCSetCriterion (no GPU needed)."""
import ctypes
import inspect
import os
import re

import pytest
import torch

import __graft_entry__ as ge
import criterion_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def built():
    ge.build()


def _nonzero_errors(fx):
    """the reference's errors like CriterionFixture.reference_errors, over the scalars and gradient tensors whose float64 value is not 0
    everywhere (None when there is none)"""
    losses, dm, dl = fx.restated()
    el = [cc.scalar_err(fx.ref_losses[l, k], losses[l, k]) for l in range(fx.L) for k in range(3) if float(losses[l, k]) != 0.0]
    eg = [cc.grad_err(r, g) for l in range(fx.L) for r, g in ((fx.ref_dmasks[l], dm[l]), (fx.ref_dlogits[l], dl[l])) if float(g.abs().max()) != 0.0]
    return (max(el) if el else None), (max(eg) if eg else None)


@pytest.mark.parametrize("name", list(cc.CASES) + list(cc.EDGE_CASES))
def test_restatement_agrees_with_the_reference_within_the_fp32_bound(name):
    """the reference's fp32 losses and gradients lie within the format-derived bound of the float64 restatement, and not closer than
    fp32 can be (a restatement that copied the stored values would show no error at all).  An edge case may hold values that are 0 in
    float64 (no object: mask and dice loss) and then exact in fp32: there the lower bound is asked of the nonzero values."""
    fx = cc.fixture(name)
    el, eg = fx.reference_errors()
    bound = cc.fp32_bound(fx.N, fx.P, fx.K)
    print(f"{name}: reference fp32 error  losses {el:.3e}  gradients {eg:.3e}  bound {bound:.3e}")
    assert el < bound and eg < bound
    if name in cc.CASES:
        assert 2.0 ** -27 < el and 2.0 ** -27 < eg
        assert list(fx.meta["M"]) == list(cc.CASES[name][1])
    else:
        nl, ng = _nonzero_errors(fx)
        assert nl is not None and ng is not None            # every case has a class loss
        assert 2.0 ** -27 < nl and 2.0 ** -27 < ng
        N, Ms, K, T, H, W, L, share, mv, kind = cc.EDGE_CASES[name]
        m = fx.meta
        assert (m["N"], tuple(m["M"]), m["K"], m["T"], m["H"], m["W"], m["L"], m["share"], m["masking"], m["kind"]) == (N, Ms, K, T, H, W, L, share, mv, kind)


def test_edge_cases_have_the_properties_they_are_there_for():
    """what tests/criterion_cases.py says of each edge case holds for the stored fixture (a seed that passed the generator's screens)"""
    fx = cc.fixture("g19_criterion_N1_M1_L1_share_mv1")
    losses, dm, _ = fx.restated()
    assert fx.P == 1 and fx.K + 1 == 2 and float(losses[0, 1]) == 0.0 and fx.meta["nonzero"] == [0]           # every ce is 0: count = max(0, 1)
    assert float(fx.ref_losses[0, 1]) == 0.0
    fx = cc.fixture("g19_criterion_N2_M1-3_L2_own_mv1")
    assert [len(fx.pairs[j][1][0]) for j in range(2)] == [2, 2] and fx.P == 65                                  # M = 3 > N = 2: solved on the transpose
    fx = cc.fixture("g19_criterion_N3_M2-0_L3_share_mv1_float")
    assert fx.P == 63 and fx.pairs[0][1][0].numel() == 0 and len(fx.pairs) == 1
    fx = cc.fixture("g19_criterion_N5_M0-4_L2_own_mv1")
    assert fx.pairs[0][0][0].numel() == 0 and fx.pairs[0][1][0].numel() == 4 and fx.P == 300
    fx = cc.fixture("g19_criterion_N7_M9-2_L2_share_mv0")
    assert len(fx.pairs[0][0][0]) == 7 and not fx.masking
    fx = cc.fixture("g19_criterion_N6_M0-0_L2_share_mv1")
    losses, dm, dl = fx.restated()
    assert float(losses[:, 1:].abs().max()) == 0.0 and float(losses[:, 0].min()) > 0.0                        # the class loss comes from the void IoU alone
    assert all(float(g.abs().max()) == 0.0 for g in dm) and all(float(g.abs().max()) > 0.0 for g in dl)
    for name in cc.EDGE_CASES:                                                                                   # void pixels exist wherever masking is on
        fx = cc.fixture(name)
        if fx.masking and name != "g19_criterion_N1_M1_L1_share_mv1":
            assert any(int(v.sum()) > 0 for per_video in cc.void_pixels(fx) for v in per_video), name


def test_blank_targets_leave_every_pixel_void():
    """the case without a fixture (criterion_cases.UNSCREENED_CASES): objects whose masks are all zero.  Every similarity is 0, so every
    assignment ties and none is stable; under masking every pixel is void, the mask and dice losses are exactly 0 in float64 whatever
    the pairs, and so is d pred_masks."""
    import matcher_cases as mc
    (case,) = cc.UNSCREENED_CASES.values()
    N, Ms, K, T, H, W, L, share, mv, kind = case
    layers, targets = cc.make_case(case, 0)
    assert all(t["masks"].shape == (M, T, H, W) and not bool(t["masks"].any()) for t, M in zip(targets, Ms)) and min(Ms) > 0
    for masking in (True, False):
        for b, t in enumerate(targets):
            ms, _, C, rows, cols = mc.restate(layers[0]["pred_masks"][b], layers[0]["pred_logits"][b], t["masks"], t["labels"], masking)
            assert float(ms.abs().max()) == 0.0 and float(C.abs().max()) == 0.0 and not mc.stable(C, rows, cols, trials=20)
    pairs = [[mc.restate(layers[0]["pred_masks"][b], layers[0]["pred_logits"][b], t["masks"], t["labels"], True)[3:] for b, t in enumerate(targets)]]
    ls = [{k: v.double().requires_grad_(True) for k, v in o.items()} for o in layers]
    losses = cc.criterion64(ls, targets, pairs, K, True, True)
    losses.sum().backward()
    losses = losses.detach()
    assert float(losses[:, 1:].abs().max()) == 0.0 and float(losses[:, 0].min()) > 0.0
    assert all(float(o["pred_masks"].grad.abs().max()) == 0.0 for o in ls)


def test_video_without_objects_is_all_void():
    """(5, 0): the second video's mask losses are 0 and every query's class weight is its void IoU (= sum prob / (sum prob + 1e-5))"""
    fx = cc.fixture("g19_criterion_N16_M5-0_L3_share_mv1")
    one = [{k: v[1:2].double() for k, v in o.items()} for o in fx.layers]
    losses = cc.criterion64(one, fx.targets[1:], [[p[1]] for p in fx.pairs], fx.K, True, True)
    assert float(losses[:, 1].abs().max()) == 0.0 and float(losses[:, 2].abs().max()) == 0.0
    assert float(losses[:, 0].min()) > 0.0


def test_constructor_mirrors_the_reference():
    import axial_vs_amd as ax
    assert ax.MaXTronCCSetCriterion.__module__ == "axial_vs_amd.criterion"
    sig = inspect.signature(ax.MaXTronCCSetCriterion.__init__)
    assert list(sig.parameters) == ["self", "num_classes", "matcher", "weight_dict", "eos_coef", "losses", "share_final_matching", "process_semantic",
                                    "pixel_insdis_temperature", "pixel_insdis_sample_k", "aux_semantic_temperature", "aux_semantic_sample_k",
                                    "masking_void_pixel"]
    assert [sig.parameters[k].default for k in list(sig.parameters)[7:]] == [False, 1.5, 4096, 2.0, 4096, True]
    m = ax.VideoHungarianMatcher(masking_void_pixel=False)
    wd = {"loss_ce": 3.0}
    for cls in (ax.MaXTronCCSetCriterion, ax.MaXTronWCSetCriterion):
        c = cls(19, m, wd, 0.1, ["labels", "masks"], True, masking_void_pixel=False)
        assert (c.num_classes, c.matcher, c.weight_dict, c.eos_coef, c.losses, c.share_final_matching) == (19, m, wd, 0.1, ["labels", "masks"], True)
        assert (c.process_semantic, c.pixel_insdis_temperature, c.pixel_insdis_sample_k, c.aux_semantic_temperature, c.aux_semantic_sample_k,
                c.masking_void_pixel) == (False, 1.5, 4096, 2.0, 4096, False)
    assert list(inspect.signature(ax.MaXTronCCSetCriterion.forward).parameters) == ["self", "outputs", "targets", "clip_outputs"]
    assert list(inspect.signature(ax.MaXTronWCSetCriterion.forward).parameters) == ["self", "outputs", "targets"]


@pytest.mark.parametrize("loss", ["pixels", "aux_semantic"])
def test_sampled_losses_are_refused_at_construction(loss):
    import axial_vs_amd as ax
    with pytest.raises(NotImplementedError, match="Gumbel"):
        ax.MaXTronCCSetCriterion(19, None, {}, 0.1, ["labels", "masks", loss], True)


def test_cpu_tensors_raise():
    import axial_vs_amd as ax
    fx = cc.fixture("g19_criterion_N100_M1_L1_share_mv1")
    with pytest.raises(RuntimeError, match="GPU"):
        ax.set_criterion_losses(fx.outputs(), fx.targets, fx.K)
    with pytest.raises(RuntimeError, match="GPU"):
        ax.MaXTronCCSetCriterion(fx.K, ax.VideoHungarianMatcher(), {}, 0.1, ["labels", "masks"], True)(fx.outputs(), fx.targets)


def _declared_arg_count(name):
    text = open(os.path.join(ROOT, "include", "axvs.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    args = re.search(r"\b" + name + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
    return len([a for a in args.split(",") if a.strip()])


def test_entry_points_are_bound_and_refuse_bad_arguments_before_any_device_work():
    from axial_vs_amd import _lib
    L = _lib.lib()
    for name in ("axvs_set_criterion_saved_bytes", "axvs_set_criterion_workspace_bytes", "axvs_set_criterion_fwd", "axvs_set_criterion_bwd"):
        assert hasattr(L, name)
        assert len(_lib.SIGNATURES[name][1]) == _declared_arg_count(name), name
    ws, sv = L.axvs_set_criterion_workspace_bytes, L.axvs_set_criterion_saved_bytes
    assert ws(4, 1, 128, 125, 65536) > 0 and sv(4, 1, 128) >= 4 * (9 * 128 + 2) * 4
    assert sv(4, 1, 128) < 4 * 128 * 65536 // 1000                      # O(L B N): nothing like a [N, P] map
    assert ws(4, 1, 513, 125, 65536) == 0 and b"512" in L.axvs_last_error()
    assert sv(17, 1, 128) == 0 and ws(1, 65, 128, 125, 64) == 0 and ws(1, 1, 128, 1, 64) == 0 and ws(1, 1, 128, 125, 0) == 0
    one = (ctypes.c_void_p * 1)(16)
    m1 = (ctypes.c_int * 1)(5)

    def fwd(masks=one, logits=one, tgt=16, tdt=_lib.AXVS_U8, labels=16, m=m1, rows=16, kmax=5, Ln=1, B=1, N=16, K1=8, P=120, losses=16, saved=16,
            wsp=16, wsb=1 << 30):
        return L.axvs_set_criterion_fwd(masks, logits, tgt, tdt, labels, m, rows, 16, 16, 16, kmax, Ln, B, N, K1, P, 1, 1, losses, saved, wsp, wsb, None)

    for kw in (dict(masks=None), dict(logits=None), dict(m=None), dict(tgt=None), dict(labels=None), dict(rows=None), dict(losses=None),
               dict(saved=None), dict(wsp=None), dict(masks=(ctypes.c_void_p * 1)(None))):
        assert fwd(**kw) == -1 and b"null" in L.axvs_last_error(), kw
    for kw in (dict(Ln=0), dict(Ln=17), dict(B=0), dict(B=65), dict(N=0), dict(N=513), dict(K1=1), dict(P=0), dict(tdt=0), dict(kmax=17),
               dict(m=(ctypes.c_int * 1)(513))):
        assert fwd(**kw) == -1, kw
    assert fwd(wsb=16) == -2 and b"workspace" in L.axvs_last_error()
    assert L.axvs_set_criterion_bwd(None, one, one, 16, _lib.AXVS_U8, m1, 1, 1, 16, 8, 120, 1, 1, 16, one, one, None) == -1
    assert L.axvs_set_criterion_bwd(16, one, one, 16, _lib.AXVS_U8, m1, 1, 1, 513, 8, 120, 1, 1, 16, one, one, None) == -1
