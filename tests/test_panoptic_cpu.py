"""CPU: the screens of the video panoptic cases (tests/panoptic_cases.py), the restatement against the reference's stored results
(tests/golden/g20_panoptic_*.npz), and the C-ABI's refusals before any device work."""
import ctypes

import pytest
import torch

import __graft_entry__ as ge
import axial_vs_amd.panoptic  # noqa: F401  (the module under test)
import panoptic_cases as pc


@pytest.fixture(scope="module", autouse=True)
def built():
    ge.build()


_STATS = {}


def _name(c):
    return "x".join(map(str, c))


@pytest.mark.parametrize("c", pc.CASES, ids=_name)
def test_the_pinned_seed_passes_every_screen(c):
    """conditions on the inputs, not tolerances: no pixel score within 8x the fp32 composition's own error of a pixel threshold,
    deciding class scores at least 1e-4 from their thresholds, reorder scores of slots with area at least 1e-5 apart, and the fp32
    composition giving the float64 map exactly -- for both scales and all three settings"""
    ok, why, st = pc.screen(c, pc.inputs_of(c))
    assert ok, why
    print(f"[panoptic screen] {pc.case_name(c)} seed {pc.pinned(c)[0]} ({len(pc.pinned(c)[1])} nudges): fp32 error {min(st['err']):.1e} .. {max(st['err']):.1e}, "
          + ", ".join(f"{k} {v}" for k, v in st.items() if k != "err"))
    # the yardstick itself is sane, an fp32 computation's error: a few ulps of a score at the small sizes; at the large one the resize's fp32
    # source coordinates (up to 327) are off by eps * 327 = 2e-5 of a logit step (up to 10), which moves a score by up to 0.25 of that
    assert 5e-8 < min(st["err"]) and max(st["err"]) < (5e-6 if c[5] < 100 else 5e-5)
    _STATS[c] = st


def test_the_case_set_shows_every_branch_of_the_merge():
    """across the cases the float64 runs show two- and three-candidate pixels, rejections by overlap and by confidence, a merged
    stuff class, a thing category with ii >= 2, and an exact tie new == orig * overlap"""
    for c in pc.CASES:
        if c not in _STATS:
            ok, why, _STATS[c] = pc.screen(c, pc.inputs_of(c))
            assert ok, why
    tot = {k: sum(s[k] for s in _STATS.values()) for k in ("two", "three", "rej_overlap", "rej_conf", "merged_stuff", "exact_tie")}
    assert all(v > 0 for v in tot.values()), tot
    assert max(s["max_ii"] for s in _STATS.values()) >= 2
    multi = _STATS[pc.MULTI_WG]
    assert multi["two"] > 0 and multi["three"] > 0          # the contested list is exercised across workgroups


@pytest.mark.parametrize("c", pc.FIXTURE_CASES, ids=_name)
def test_restatement_equals_the_reference(c):
    """the float64 restatement gives the reference's own (fp32, CPU) map, dict keys in order, list lengths and embeddings"""
    meta, inputs, ref = pc.load_fixture(c)
    assert meta["seed"] == pc.SEED0 + pc.pinned(c)[0]
    for a, b in zip(inputs, pc.inputs_of(c)):
        assert torch.equal(a, b)
    for si, sf in enumerate(pc.SCALES):
        for ti, setting in enumerate(pc.SETTINGS):
            m, d, _ = pc.restated(c, sf, setting)
            rm, keys, embs = ref[(sf, ti)]
            assert rm.dtype == torch.int32 and torch.equal(m, rm), (sf, ti)
            assert list(d) == keys and [len(v) for v in d.values()] == [len(e) for e in embs]
            for v, e in zip(d.values(), embs):
                assert float((torch.stack(v) - e.double()).abs().max()) <= 1e-6


def _cfg(**kw):
    from axial_vs_amd import _lib
    base = dict(N=16, K1=8, T=2, h=6, w=10, image_h=24, image_w=40, two_stage=0, crop_h=0, crop_w=0, H=22, W=39, align_corners=0, label_divisor=1000,
                pixel_confidence_threshold=0.4, overlap_threshold=0.8, class_threshold_thing=0.7, class_threshold_stuff=0.5, reorder_class_weight=1.0,
                reorder_mask_weight=1.0)
    base.update(kw)
    return _lib.AxvsPanopticCfg(**base)


def test_cabi_refuses_bad_arguments_without_a_device():
    from axial_vs_amd import _lib
    L = _lib.lib()
    p = [ctypes.c_void_p(0x10000 * (i + 1)) for i in range(8)]           # made-up pointers: every check comes before any device work

    def call(cfg, ws_bytes, ptrs=p):
        return L.axvs_video_panoptic_fwd(ctypes.byref(cfg), ptrs[0], ptrs[1], _lib.AXVS_F32, ptrs[2], ptrs[3], ptrs[4], ptrs[5], ptrs[6], ptrs[7],
                                         ws_bytes, None)
    good = _cfg()
    need = L.axvs_video_panoptic_workspace_bytes(ctypes.byref(good))
    assert need >= 2 * 22 * 39 * 8 and L.axvs_video_panoptic_table_ints(16) == 4 + 7 * 16
    for bad, word in ((_cfg(N=513), "512"), (_cfg(pixel_confidence_threshold=0.25), "0.25"), (_cfg(pixel_confidence_threshold=0.2), "0.25"),
                      (_cfg(pixel_confidence_threshold=1.0), "0.25"), (_cfg(H=25), "crop"), (_cfg(two_stage=1, crop_h=25, crop_w=10), "crop"),
                      (_cfg(T=1 << 12, H=1 << 10, W=1 << 9, image_h=1 << 10, image_w=1 << 9), "2^31")):
        assert L.axvs_video_panoptic_workspace_bytes(ctypes.byref(bad)) == 0
        assert word in L.axvs_last_error().decode()
        assert call(bad, 1 << 40) == -1 and word in L.axvs_last_error().decode()
    assert call(good, need - 1) == -2
    err = L.axvs_last_error().decode()
    assert "workspace too small" in err and str(need - 1) in err and str(need) in err
    for i in range(8):                                                    # a null pointer in any position
        q = list(p)
        q[i] = None
        assert call(good, need, q) == -1 and "null" in L.axvs_last_error().decode()
    assert L.axvs_video_panoptic_fwd(None, p[0], p[1], _lib.AXVS_F32, *p[2:], need, None) == -1
    assert L.axvs_video_panoptic_fwd(ctypes.byref(good), p[0], p[1], _lib.AXVS_U8, *p[2:], need, None) == -1


def test_python_entry_point_refuses_cpu_tensors():
    import axial_vs_amd as ax
    c = pc.CASES[0]
    mp, cls, emb = pc.inputs_of(c)
    things, stuff = pc.ids_of(c[6])
    post = ax.VideoPanopticPostProcessor(things, stuff, pc.LABEL_DIVISOR, 0.7, 0.5, 0.4, 0.8, 1.0, 1.0)
    g = pc.geometry(c, 1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        post(cls, mp, emb, g.ac, g.image_h, g.image_w, g.sf, g.scaled_h, g.scaled_w, g.height, g.width)
