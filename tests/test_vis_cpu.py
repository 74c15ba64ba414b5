"""CPU: the screens of the video instance cases (tests/vis_cases.py), the restatement against the reference's stored results
(tests/golden/g21_vis_*.npz), the new entry points' declarations, and the C-ABI's refusals before any device work."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
import vis_cases as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def built():
    ge.build()


_STATS = {}


def _screened(c):
    if c not in _STATS:
        ok, why, _STATS[c] = vc.screen(c, vc.inputs_of(c))
        assert ok, why
    return _STATS[c]


@pytest.mark.parametrize("c", vc.CASES, ids=lambda c: c.name)
def test_the_pinned_seed_passes_every_screen(c):
    """conditions on the inputs, not tolerances: no resized float64 logit of a candidate within 8x the fp32 restatement's own error of
    0, the top K_cand + 1 class scores and each frame's non-zero detection scores 1e-5 apart, the fp32 restatement giving the float64
    masks, candidates and selection exactly"""
    st = _screened(c)
    print(f"[vis screen] {vc.case_name(c)} seed {vc.pinned(c)[0]} ({len(vc.pinned(c)[1])} nudges): " + ", ".join(f"{k} {v:.3g}" for k, v in st.items()))
    # the yardstick itself is sane, an fp32 computation's error: the resize's fp32 source coordinates (up to 320) are off by up to
    # eps * 320 = 2e-5 of a logit step (up to 30 between neighbours), the scores by a few ulps of 1
    assert 1e-8 < st["err"] < 5e-5 and 1e-9 < st["ms_err"] < 1e-6 and st["det_err"] < 1e-6 and st["cls_err"] < 1e-6


def test_seeds_tried_stay_within_the_budget_and_only_the_multi_tile_cases_are_nudged():
    for c in vc.CASES:
        seed, nudges = vc.pinned(c)
        assert 0 <= seed < vc.MAX_SEEDS
        assert not nudges or c in vc.NUDGED


def test_the_case_set_shows_shared_queries_empty_masks_and_the_zero_score_tie():
    st = {c.name: _screened(c) for c in vc.CASES}
    assert st["d"]["shared"] >= 50 and st["d"]["empty_cands"] > 0               # half the candidates share queries; empty masks among them
    for n in ("a", "c25"):                                                      # zero scores selected while other zero scores are not:
        c = vc.BY_NAME[n]                                                       # the tie rule decides
        assert 0 < st[n]["zero_selected"] < st[n]["empty_cands"], (n, st[n])
    assert st["c25"]["ncand"] < vc.BY_NAME["c25"].K and st["c"]["ncand"] == 100  # the thing filter drops candidates only there
    r = vc.restated(vc.BY_NAME["c25"])
    assert bool((r.label < 25).all()) and bool((vc.restated(vc.BY_NAME["c"]).label >= 25).any())
    b16, h, k = vc.BY_NAME["b16"], vc.BY_NAME["h"], vc.BY_NAME["k"]
    mp = vc.inputs_of(b16)[1]
    assert torch.equal(mp, mp.bfloat16().float()) and not torch.equal(vc.inputs_of(vc.BY_NAME["b"])[1], vc.inputs_of(vc.BY_NAME["b"])[1].bfloat16().float())
    assert -(-h.ori[0] // 4) * -(-h.ori[1] // 64) * h.F > 2048 and k.Q * k.C > 4096      # several tiles per workgroup; keys beyond the LDS table
    g, b = vc.BY_NAME["g"], vc.BY_NAME["b"]
    assert g.F == 3 < g.T and g[1:3] + g[4:11] == b[1:3] + b[4:11]


@pytest.mark.parametrize("c", vc.FIXTURE_CASES, ids=lambda c: c.name)
def test_restatement_equals_the_reference(c):
    """the reference's own run (fp32, CPU; its own 30 rows per frame) against the fp32 restatement: the rows with a non-zero score agree
    in order, (query, label), box, score and mask -- exactly; every zero-score row of the reference is an empty mask with a zero box
    (which of them it keeps is open: its argsort is not stable)"""
    meta, inputs, frames = vc.load_fixture(c)
    assert meta["seed"] == vc.SEED0 + vc.pinned(c)[0]
    for a, b in zip(inputs, vc.inputs_of(c)):
        assert torch.equal(a, b)
    r = vc.restated(c, torch.float32)
    for t, ref in enumerate(frames):
        f = r.frames[t]
        sel = torch.argsort(f.det_score, descending=True, stable=True)[:30]
        assert len(ref.rows) == len(sel)
        n = int((ref.rows[:, 7] != 0).sum())
        assert n == int((f.det_score[sel] != 0).sum())
        s = sel[:n]
        assert np.array_equal(ref.rows[:n, 1], r.query[s].numpy()) and np.array_equal(ref.rows[:n, 2], r.label[s].numpy())
        assert np.array_equal(ref.rows[:n, 3:7], f.bbox[s].numpy().astype(np.float64))
        assert np.array_equal(ref.rows[:n, 7].astype(np.float32), f.det_score[s].numpy())
        assert np.array_equal(ref.masks[:n], f.binary[s].numpy())
        assert not ref.masks[n:].any() and not ref.rows[n:, 3:].any()


def test_the_float64_restatement_selects_what_the_fp32_one_does():
    for c in vc.CASES:
        r64, r32 = vc.restated(c), vc.restated(c, torch.float32)
        assert torch.equal(r64.flat, r32.flat)
        for a, b in zip(r64.frames, r32.frames):
            assert torch.equal(a.sel, b.sel) and torch.equal(a.area, b.area) and torch.equal(a.bbox, b.bbox)


def _declared_arg_count(name):
    text = open(os.path.join(ROOT, "include", "axvs.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    args = re.search(r"\b" + name + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
    return len([a for a in args.split(",") if a.strip()])


def test_entry_points_are_importable_declared_exported_and_bound():
    import axial_vs_amd as ax
    from axial_vs_amd import _lib
    assert callable(ax.video_instance_inference) and callable(ax.VideoInstancePostProcessor) and callable(ax.unpack_bits)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("axvs_video_instance_workspace_bytes", "axvs_video_instance_fwd"):
        assert hasattr(raw, name) and hasattr(_lib.lib(), name)
        assert len(_lib.SIGNATURES[name][1]) == _declared_arg_count(name), name
    post = ax.VideoInstancePostProcessor.from_model(type("M", (), {"panoptic_fusion_head": type("H", (), {"num_things_classes": 40, "test_cfg": {"max_per_image": 100}})}))
    assert (post.num_things_classes, post.max_per_image, post.keep_per_frame) == (40, 100, 30)


def _cfg(**kw):
    from axial_vs_amd import _lib
    base = dict(Q=16, K1=8, T=2, num_frames=2, h=6, w=10, image_h=24, image_w=40, crop_h=22, crop_w=37, H=45, W=75, num_things=7, k_cand=20, k_out=5,
                mask_bits=0)
    base.update(kw)
    return _lib.AxvsVisCfg(**base)


def test_cabi_refuses_bad_arguments_without_a_device():
    from axial_vs_amd import _lib
    L = _lib.lib()
    p = [ctypes.c_void_p(0x10000 * (i + 1)) for i in range(6)]           # made-up pointers: every check comes before any device work

    def call(cfg, ws_bytes, ptrs=p):
        return L.axvs_video_instance_fwd(ctypes.byref(cfg), ptrs[0], ptrs[1], _lib.AXVS_F32, ptrs[2], ptrs[3], ptrs[4], ptrs[5], ws_bytes, None)
    good = _cfg()
    need = L.axvs_video_instance_workspace_bytes(ctypes.byref(good))
    assert need >= 16 * 7 * 8 + 2 * 16 * (8 + 4 + 16)
    for bad, word in ((_cfg(Q=513), "512"), (_cfg(Q=512, K1=258), "2^17"), (_cfg(k_cand=113), "max_per_image"), (_cfg(k_cand=257, Q=64), "max_per_image"),
                      (_cfg(k_out=21), "keep_per_frame"), (_cfg(k_out=0), "keep_per_frame"), (_cfg(num_frames=3), "num_frames"),
                      (_cfg(num_frames=0), "num_frames"), (_cfg(crop_h=25), "img_shape"), (_cfg(h=0), "positive"), (_cfg(K1=1), "class logits"),
                      (_cfg(H=1 << 16, W=1 << 15), "2^31")):
        assert L.axvs_video_instance_workspace_bytes(ctypes.byref(bad)) == 0
        assert word in L.axvs_last_error().decode(), (word, L.axvs_last_error())
        assert call(bad, 1 << 40) == -1 and word in L.axvs_last_error().decode()
    assert call(good, need - 1) == -2
    err = L.axvs_last_error().decode()
    assert "workspace too small" in err and str(need - 1) in err and str(need) in err
    for i in range(6):                                                    # a null pointer in any position
        q = list(p)
        q[i] = None
        assert call(good, need, q) == -1 and "null" in L.axvs_last_error().decode()
    assert L.axvs_video_instance_fwd(None, p[0], p[1], _lib.AXVS_F32, *p[2:], need, None) == -1
    assert L.axvs_video_instance_fwd(ctypes.byref(good), p[0], p[1], _lib.AXVS_U8, *p[2:], need, None) == -1


def test_python_entry_point_refuses_cpu_tensors():
    import axial_vs_amd as ax
    c = vc.BY_NAME["a"]
    cls, mp = vc.inputs_of(c)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ax.video_instance_inference(cls, mp, batch_input_shape=c.bi, img_shape=c.img, ori_shape=c.ori, num_things_classes=c.things,
                                    max_per_image=c.K, keep_per_frame=c.Ko)


def test_unpack_bits_follows_the_documented_bit_order():
    import axial_vs_amd as ax
    w = torch.zeros(2, 2, dtype=torch.int64)
    w[0, 0], w[0, 1], w[1, 0] = 0b101, 1 << 2, -(1 << 63)                 # pixels 0 and 2; pixel 66; pixel 63
    for got in (ax.unpack_bits(w, 70).numpy(), ax.unpack_bits(w.numpy(), 70)):
        assert got.shape == (2, 70) and got.dtype == bool
        assert np.flatnonzero(got[0]).tolist() == [0, 2, 66] and np.flatnonzero(got[1]).tolist() == [63]
