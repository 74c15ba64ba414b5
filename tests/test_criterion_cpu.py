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


@pytest.mark.parametrize("name", list(cc.CASES))
def test_restatement_agrees_with_the_reference_within_the_fp32_bound(name):
    """the reference's fp32 losses and gradients lie within the format-derived bound of the float64 restatement, and not closer than
    fp32 can be (a restatement that copied the stored values would show no error at all)"""
    fx = cc.fixture(name)
    el, eg = fx.reference_errors()
    bound = cc.fp32_bound(fx.N, fx.P, fx.K)
    print(f"{name}: reference fp32 error  losses {el:.3e}  gradients {eg:.3e}  bound {bound:.3e}")
    assert 2.0 ** -27 < el < bound
    assert 2.0 ** -27 < eg < bound
    assert list(fx.meta["M"]) == list(cc.CASES[name][1])


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
