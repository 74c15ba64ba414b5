"""CPU: the float64 restatement of Tube-Link's point-sampled loss against the reference's stored fp32 results, the order and shapes of
`draw_point_coords`, the screens of every case (tests/tl_loss_cases.py), and the host-side surface of axvs_tl_loss_* and
TubeLinkSetCriterion (argument errors, size functions, refused configurations)."""
import ctypes

import pytest
import torch

import __graft_entry__ as ge
import tl_loss_cases as tc

NAMES = list(tc.CASES)


@pytest.fixture(scope="module", autouse=True)
def built():
    ge.build()


def fp32_bound(c):
    """derived from the number format (u = 2^-24), as in criterion_cases: a bilinear sample is four products and three sums (8 u), a
    softplus / sigmoid / softmax value a few roundings more, a sum of P such terms at most (P - 1) u more in any order, a ratio of two
    sums twice that plus the division, and a loss or a cost entry is a short weighted sum of such ratios over Q or K + 1 terms:
    4 (P + Q + K + 16) u, relative to the value (a scalar) or to the largest entry (a matrix, a gradient)."""
    return 4.0 * (c["P"] + c["Q"] + c["K"] + 16) * tc.U32


@pytest.mark.parametrize("name", NAMES)
def test_restatement_agrees_with_the_reference_fixture(name):
    fx = tc.fixture(name)
    c, r = fx.c, fx.restated()
    L, B = c["L"], len(c["M"])
    bound = fp32_bound(c)
    for l in range(L):
        for b in range(B):
            assert torch.equal(r["rows"][l][b], fx.ref_pairs[l][b][0]) and torch.equal(r["cols"][l][b], fx.ref_pairs[l][b][1]), (l, b)
            assert len(r["rows"][l][b]) == min(c["Q"], c["M"][b])
            if c["M"][b] > 0:
                assert tc.tensor_err(fx.ref_cost[l][b], r["cost"][l][b]) <= bound
        if fx.ref_selected is not None:
            assert torch.equal(r["selected"][l], fx.ref_selected[l]), l
        for j in range(3):
            assert tc.scalar_err(fx.ref_losses[l, j], r["losses"][l, j]) <= bound, (l, j)
        assert tc.tensor_err(fx.ref_dcls[l], r["dcls"][l]) <= bound
        assert tc.tensor_err(fx.ref_dmasks[l], fx.sub(r["dmasks"][l])) <= bound


@pytest.mark.parametrize("name", NAMES)
def test_draw_point_coords_reproduces_the_recorded_draws(name):
    """the reference's torch.rand calls under the fixture's seed, recorded by shape and SHA-256: per layer (1, P, 2) per video, then
    (G, S, 2), then (G, P - k, 2) when P - k > 0; nothing after the per-video draws when no query is matched"""
    import axial_vs_amd as ax
    fx = tc.fixture(name)
    c = fx.c
    S, k, G = tc.counts(c)
    gen = torch.Generator().manual_seed(fx.seed + 1)
    match, cand, rand = ax.draw_point_coords(c["L"], c["M"], c["Q"], c["P"], c["over"], c["ratio"], "cpu", generator=gen)
    assert match.shape == (c["L"], len(c["M"]), c["P"], 2) and cand.shape == (c["L"], G, S, 2) and rand.shape == (c["L"], G, c["P"] - k, 2)
    mine = []
    for l in range(c["L"]):
        mine += [match[l, b][None] for b in range(len(c["M"]))]
        if G > 0:
            mine.append(cand[l])
            if c["P"] - k > 0:
                mine.append(rand[l])
    rec = fx.meta["draws"]
    assert [list(t.shape) for t in mine] == [d["shape"] for d in rec]
    assert [tc.digest(t) for t in mine] == [d["sha256"] for d in rec]


@pytest.mark.parametrize("name", NAMES)
def test_screens_hold_at_the_fixed_seed(name):
    fx = tc.fixture(name)
    assert fx.seed == fx.meta["seed"] and set(tc.seeds()) == set(tc.CASES)
    stable, wide, worst = tc.screens(fx.c, fx.inp, fx.coords, fx.restated())
    print(f"[tl_loss] {name}: seed {fx.seed}, smallest selection gap / (8 x fp32 error) = {worst:.3g}")
    assert stable and wide


def test_case_list_covers_what_it_names():
    cs = tc.CASES.values()
    assert {c["Q"] for c in cs} >= {5, 33, 100} and {m for c in cs for m in c["M"]} >= {0, 1, 3}
    assert any(c["M"][0] == c["Q"] for c in cs) and any(c["M"][0] > c["Q"] for c in cs)
    assert any(len(c["M"]) == 2 and 0 in c["M"] for c in cs) and {c["L"] for c in cs} >= {1, 3} and {c["T"] for c in cs} >= {1, 2, 3}
    assert {(c["h"], c["w"]) for c in cs} >= {(7, 9), (12, 20)} and {c["gs"] for c in cs} >= {1, 4} and {c["kind"] for c in cs} == {"u8", "f32"}
    assert {c["P"] for c in cs} >= {64, 112, 12544}
    assert {(c["over"], c["ratio"]) for c in cs} >= {(3.0, 0.75), (3.0, 0.0), (1.0, 1.0), (1.5, 0.5)}
    for c in cs:      # frame boundaries fall inside the sampled range: the long image has T*h rows and the points cover [0, 1)
        assert c["T"] * c["h"] <= 8192


# ---- the host-side surface ----------------------------------------------------------------------------------------------------------------
def _cfg(**kw):
    from axial_vs_amd import _lib
    base = dict(L=1, B=1, Q=5, K1=5, T=2, h=7, w=9, Hg=7, Wg=9, num_points=64, num_cand=192, num_kept=48, target_dtype=_lib.AXVS_U8,
                cost_cls=2, cost_mask=5, cost_dice=5, loss_cls=2, loss_mask=5, loss_dice=5, dice_eps=1)
    base.update(kw)
    return _lib.AxvsTLLossCfg(**base)


def test_size_functions_need_no_gpu_and_grow_with_the_pairs():
    from axial_vs_amd import _lib
    L = _lib.lib()
    m3, m0 = (ctypes.c_int * 1)(3), (ctypes.c_int * 1)(0)
    s3, s0 = L.axvs_tl_loss_saved_bytes(_cfg(), m3), L.axvs_tl_loss_saved_bytes(_cfg(), m0)
    assert s0 > 0 and s3 >= s0 + 3 * 64 * 2 * 4          # the chosen coordinates of three pairs
    assert L.axvs_tl_loss_workspace_bytes(_cfg(), m3) >= 5 * 3 * 4 and L.axvs_tl_loss_workspace_bytes(_cfg(), m0) > 0


@pytest.mark.parametrize("kw, m, word", [
    (dict(L=17), 3, "L=17"), (dict(L=0), 3, "L=0"), (dict(B=65), 3, "B=65"), (dict(Q=513), 3, "Q=513"), (dict(), 513, "m_per_video[0]=513"),
    (dict(), -1, "m_per_video[0]=-1"), (dict(num_points=16385), 3, "num_points=16385"), (dict(num_cand=65537), 3, "S=65537"),
    (dict(num_kept=65), 3, "k=65"), (dict(num_kept=200, num_points=256), 3, "k=200"), (dict(K1=1), 3, "K + 1 = 1"),
    (dict(T=1200, h=7), 3, "T*h=8400"), (dict(target_dtype=0), 3, "target dtype 0"),
])
def test_bounds_are_refused_by_name(kw, m, word):
    from axial_vs_amd import _lib
    L = _lib.lib()
    B = kw.get("B", 1)
    mv = (ctypes.c_int * max(B, 1))(*([m] * max(B, 1)))
    cfg = _cfg(**kw)
    for query in (L.axvs_tl_loss_saved_bytes, L.axvs_tl_loss_workspace_bytes):
        assert query(cfg, mv) == 0
        assert word in L.axvs_last_error().decode(), L.axvs_last_error().decode()
    p = [ctypes.c_void_p(0x10000 * (i + 1)) for i in range(16)]
    arr = (ctypes.c_void_p * 16)(*[0x100000] * 16)
    rc = L.axvs_tl_loss_fwd(cfg, arr, arr, p[0], p[1], mv, p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9], None, None, p[10], p[11], 1 << 40, None)
    assert rc == -1 and word in L.axvs_last_error().decode()
    rc = L.axvs_tl_loss_bwd(cfg, p[0], arr, arr, p[1], mv, p[2], p[3], p[4], arr, arr, None)
    assert rc == -1 and word in L.axvs_last_error().decode()


def test_null_pointers_and_a_short_workspace_are_refused_before_any_device_work():
    from axial_vs_amd import _lib
    L = _lib.lib()
    mv = (ctypes.c_int * 1)(3)
    cfg = _cfg()
    p = [ctypes.c_void_p(0x10000 * (i + 1)) for i in range(16)]
    arr = (ctypes.c_void_p * 16)(*[0x100000] * 16)
    need = L.axvs_tl_loss_workspace_bytes(cfg, mv)
    rc = L.axvs_tl_loss_fwd(cfg, arr, arr, p[0], p[1], mv, p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9], None, None, p[10], p[11], need - 1, None)
    assert rc == -2 and f"{need - 1} < {need}" in L.axvs_last_error().decode()
    rc = L.axvs_tl_loss_fwd(cfg, arr, arr, None, p[1], mv, p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9], None, None, p[10], p[11], need, None)
    assert rc == -1 and "null pointer" in L.axvs_last_error().decode()
    null_layer = (ctypes.c_void_p * 16)(*[None] * 16)
    rc = L.axvs_tl_loss_fwd(cfg, null_layer, arr, p[0], p[1], mv, p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9], None, None, p[10], p[11], need, None)
    assert rc == -1 and "layer 0" in L.axvs_last_error().decode()
    rc = L.axvs_tl_loss_bwd(cfg, None, arr, arr, p[1], mv, p[2], p[3], p[4], arr, arr, None)
    assert rc == -1 and "null pointer" in L.axvs_last_error().decode()


HEAD_CFG = dict(
    loss_cls=dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=2.0, reduction="mean", class_weight=[1.0] * 4 + [0.1]),
    loss_mask=dict(type="CrossEntropyLoss", use_sigmoid=True, reduction="mean", loss_weight=5.0),
    loss_dice=dict(type="DiceLoss", use_sigmoid=True, activate=True, reduction="mean", naive_dice=True, eps=1.0, loss_weight=5.0),
    train_cfg=dict(num_points=64, oversample_ratio=3.0, importance_sample_ratio=0.75,
                   assigner=dict(type="MaskHungarianAssigner", cls_cost=dict(type="ClassificationCost", weight=2.0),
                                 mask_cost=dict(type="CrossEntropyLossCost", weight=5.0, use_sigmoid=True),
                                 dice_cost=dict(type="DiceCost", weight=5.0, pred_act=True, eps=1.0)),
                   sampler=dict(type="MaskPseudoSampler")))


def test_criterion_takes_the_heads_config_and_refuses_what_is_not_built():
    import copy

    import axial_vs_amd as ax
    crit = ax.TubeLinkSetCriterion(4, **HEAD_CFG)
    assert crit.cost_weights == (2.0, 5.0, 5.0) and crit.loss_weights == (2.0, 5.0, 5.0) and crit.num_points == 64 and crit.dice_eps == 1.0
    assert crit.class_weight == [1.0] * 4 + [0.1]
    with pytest.raises(NotImplementedError, match="point_loss"):
        ax.TubeLinkSetCriterion(4, point_loss=False, **HEAD_CFG)
    for path, key, value in [(("loss_cls",), "use_sigmoid", True), (("loss_mask",), "type", "FocalLoss"), (("loss_dice",), "naive_dice", False),
                             (("train_cfg", "assigner", "dice_cost"), "pred_act", False), (("train_cfg", "assigner", "cls_cost"), "type", "FocalLossCost"),
                             (("train_cfg", "assigner"), "type", "HungarianAssigner"), (("train_cfg", "assigner", "dice_cost"), "eps", 1e-3)]:
        cfg = copy.deepcopy(HEAD_CFG)
        d = cfg
        for p in path:
            d = d[p]
        d[key] = value
        with pytest.raises(NotImplementedError, match=key if key != "eps" else "eps"):
            ax.TubeLinkSetCriterion(4, **cfg)


def test_there_is_no_cpu_fallback_and_no_16_bit_tier():
    import axial_vs_amd as ax
    cls, masks = torch.zeros(1, 1, 5, 5), torch.zeros(1, 1, 2, 5, 7, 9)
    labels, gt = [torch.zeros(2, dtype=torch.int64)], [torch.zeros(2, 2, 7, 9, dtype=torch.uint8)]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ax.tube_link_losses(cls, masks, labels, gt, num_classes=4, class_weight=[1.0] * 5, num_points=64)
    with pytest.raises(NotImplementedError, match="fp32"):
        ax.tube_link_losses(cls.half(), masks.half(), labels, gt, num_classes=4, class_weight=[1.0] * 5, num_points=64)
