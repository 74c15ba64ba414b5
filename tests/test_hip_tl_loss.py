"""GPU: Tube-Link's point-sampled training loss (axial_vs_amd.tube_link_losses / axvs_tl_loss_*) against the float64 restatement and the
reference's fixtures, with the reference's own fp32 error as the yardstick (tests/tl_loss_cases.py).

Measured device error / reference error per case and quantity: profiles/tl_loss_parity.txt."""
import ctypes

import pytest
import torch

import __graft_entry__ as ge
import tl_loss_cases as tc

pytestmark = pytest.mark.gpu
MARGIN = 8.0
NAMES = [n for n in tc.CASES if not tc.CASES[n].get("hand")]


@pytest.fixture(scope="module", autouse=True)
def built():
    ge.build()
    assert torch.cuda.is_available()


def _call(fx, requires_grad=True):
    import axial_vs_amd as ax
    c, inp = fx.c, fx.inp
    cls = [t.cuda().requires_grad_(requires_grad) for t in inp["cls"]]
    masks = [t.cuda().requires_grad_(requires_grad) for t in inp["masks"]]
    losses, info = ax.tube_link_losses(cls, masks, [t.cuda() for t in inp["labels"]], [t.cuda() for t in inp["gt"]], num_classes=c["K"],
                                       class_weight=inp["class_weight"], num_points=c["P"], oversample_ratio=c["over"],
                                       importance_sample_ratio=c["ratio"], cost_weights=tc.COST_W, loss_weights=tc.LOSS_W, dice_eps=tc.DICE_EPS,
                                       point_coords=[t.cuda() for t in fx.coords], return_assignment=True)
    return cls, masks, losses, info


def _run(fx):
    """forward, device-side weighted sum, backward -> dict(losses [L, 3], info, dcls, dmasks)"""
    L = fx.c["L"]
    cls, masks, losses, info = _call(fx)
    assert list(losses) == tc.loss_keys(L)
    w = torch.tensor(tc.upstream_weights(L), device="cuda", dtype=torch.float32)
    pos = tc.layer_of_key(L)
    arr = torch.stack([losses[k] for k in tc.loss_keys(L)])
    (arr * w[pos]).sum().backward()
    out = torch.zeros(3 * L)
    out[pos] = arr.detach().cpu()
    return dict(losses=out.reshape(L, 3), info=info, dcls=[t.grad.cpu() for t in cls], dmasks=[t.grad.cpu() for t in masks])


_runs = {}


def _shared_run(name):
    if name not in _runs:
        _runs[name] = _run(tc.fixture(name))
    return _runs[name]


def _pairs_of(info, c, l, b):
    Q, B = c["Q"], len(c["M"])
    n = min(Q, c["M"][b])
    rows, cols = info["rows"].cpu(), info["cols"].cpu()
    if rows.shape[1] > n:
        assert bool((rows[l * B + b, n:] == -1).all()) and bool((cols[l * B + b, n:] == -1).all())
    return rows[l * B + b, :n], cols[l * B + b, :n]


def _compare(fx, got):
    """assignments and kept sets equal; -> error / yardstick per quantity"""
    c, r, yard = fx.c, fx.restated(), fx.yard()
    L, B = c["L"], len(c["M"])
    S, k, G = tc.counts(c)
    ec = 0.0
    for l in range(L):
        for b in range(B):
            rows, cols = _pairs_of(got["info"], c, l, b)
            assert torch.equal(rows, r["rows"][l][b]) and torch.equal(cols, r["cols"][l][b]), (l, b)
            assert torch.equal(rows, fx.ref_pairs[l][b][0]) and torch.equal(cols, fx.ref_pairs[l][b][1]), (l, b)
            if c["M"][b] > 0:
                ec = max(ec, tc.tensor_err(got["info"]["cost"][l * B + b, :, :c["M"][b]], r["cost"][l][b]))
        if G > 0 and k > 0:
            sel = got["info"]["selected"][l].cpu().long()
            assert bool((sel[:, 1:] > sel[:, :-1]).all()), "kept candidates are stored in increasing order"
            assert torch.equal(sel, r["selected"][l]), l
            if fx.ref_selected is not None:
                assert torch.equal(sel, fx.ref_selected[l]), l
    el = max(tc.scalar_err(got["losses"][l, j], r["losses"][l, j]) for l in range(L) for j in range(3))
    egc = max(tc.tensor_err(got["dcls"][l], r["dcls"][l]) for l in range(L))
    egm = max(tc.tensor_err(got["dmasks"][l], r["dmasks"][l]) for l in range(L))
    ratios = dict(cost=ec / yard["cost"], losses=el / yard["losses"], dcls=egc / yard["dcls"], dmasks=egm / yard["dmasks"])
    print(f"[tl_loss] {fx.name}: " + ";  ".join(f"{q} {ratios[q]:.2f} x reference ({yard[q]:.3e})" for q in ratios))
    return ratios


@pytest.mark.parametrize("name", NAMES)
def test_assignments_selection_losses_and_gradients_match_float64(name):
    fx = tc.fixture(name)
    ratios = _compare(fx, _shared_run(name))
    for q, v in ratios.items():
        assert v <= MARGIN, (q, v)


@pytest.mark.parametrize("name", ["Q5_M5-0_L3", "Q33_M3-1_kS", "Q100_M8_big"])
def test_two_runs_are_bit_equal(name):
    a, b = _shared_run(name), _run(tc.fixture(name))
    assert torch.equal(a["losses"], b["losses"])
    for x, y in zip(a["dcls"] + a["dmasks"], b["dcls"] + b["dmasks"]):
        assert torch.equal(x, y)


@pytest.mark.parametrize("name", NAMES)
def test_unmatched_queries_have_exactly_zero_mask_gradient(name):
    fx = tc.fixture(name)
    c, r, got = fx.c, fx.restated(), _shared_run(name)
    for l in range(c["L"]):
        for b in range(len(c["M"])):
            keep = torch.ones(c["Q"], dtype=torch.bool)
            keep[r["rows"][l][b]] = False
            assert bool((got["dmasks"][l][b][:, keep] == 0).all()), (l, b)
            if len(r["rows"][l][b]):
                assert float(got["dmasks"][l][b][:, ~keep].abs().max()) > 0


def test_zero_match_layer_gives_zero_mask_and_dice_losses():
    got = _shared_run("Q33_M0")
    assert float(got["losses"][0, 1]) == 0.0 and float(got["losses"][0, 2]) == 0.0 and float(got["losses"][0, 0]) > 0
    assert bool((got["dmasks"][0] == 0).all()) and float(got["dcls"][0].abs().max()) > 0
    assert got["info"]["rows"].shape == (1, 0)


def test_no_host_synchronisation():
    """drawing the coordinates, the forward and the backward of a step with an empty video, under torch's sync debug mode"""
    import axial_vs_amd as ax
    fx = tc.fixture("Q5_M5-0_L3")
    c, inp = fx.c, fx.inp
    crit = ax.TubeLinkSetCriterion(c["K"], loss_cls=dict(type="CrossEntropyLoss", class_weight=[float(x) for x in inp["class_weight"]]),
                                   train_cfg=dict(num_points=c["P"], oversample_ratio=c["over"], importance_sample_ratio=c["ratio"]))
    cls = [t.cuda().requires_grad_(True) for t in inp["cls"]]
    masks = [t.cuda().requires_grad_(True) for t in inp["masks"]]
    labels, gt = [t.cuda() for t in inp["labels"]], [t.cuda() for t in inp["gt"]]
    gen = torch.Generator(device="cuda").manual_seed(3)
    sum(crit.loss(cls, masks, labels, gt, generator=gen).values()).backward()      # (first call: allocator, workspace, module loading)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        sum(crit.loss(cls, masks, labels, gt, generator=gen).values()).backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert masks[0].grad is not None and cls[2].grad is not None


def test_hand_placed_coordinates_through_the_c_abi():
    """0.0, the largest float below 1.0, pixel centres and the frame boundary of the long image, straight through axvs_tl_loss_fwd / _bwd:
    out-of-range taps contribute zero and a sample at the boundary blends the two frames"""
    from axial_vs_amd import _lib
    fx = tc.fixture("hand_placed")
    c, inp, r, yard = fx.c, fx.inp, fx.restated(), fx.yard()
    L, Q, K1, T, h, w, P = c["L"], c["Q"], c["K"] + 1, c["T"], c["h"], c["w"], c["P"]
    S, k, G = tc.counts(c)
    M = c["M"][0]
    lib = _lib.lib()
    cfg = _lib.AxvsTLLossCfg(L=L, B=1, Q=Q, K1=K1, T=T, h=h, w=w, Hg=h, Wg=w, num_points=P, num_cand=S, num_kept=k, target_dtype=_lib.AXVS_U8,
                             cost_cls=tc.COST_W[0], cost_mask=tc.COST_W[1], cost_dice=tc.COST_W[2], loss_cls=tc.LOSS_W[0], loss_mask=tc.LOSS_W[1],
                             loss_dice=tc.LOSS_W[2], dice_eps=tc.DICE_EPS)
    mv = (ctypes.c_int * 1)(M)
    dev = "cuda"
    cls, masks = inp["cls"][0].to(dev).contiguous(), inp["masks"][0].to(dev).contiguous()
    gt, labels, cw = inp["gt"][0].to(dev).contiguous(), inp["labels"][0].to(dev), inp["class_weight"].to(dev)
    match, cand, rand = [t.to(dev).contiguous() for t in fx.coords]
    ntm = torch.full((1,), float(max(G, 1)), device=dev)
    losses = torch.empty(L, 3, device=dev)
    rows, cols = torch.empty(1, min(Q, M), dtype=torch.int64, device=dev), torch.empty(1, min(Q, M), dtype=torch.int64, device=dev)
    cost = torch.empty(1, Q, M, device=dev)
    saved = torch.empty(lib.axvs_tl_loss_saved_bytes(cfg, mv), dtype=torch.uint8, device=dev)
    ws = torch.empty(lib.axvs_tl_loss_workspace_bytes(cfg, mv), dtype=torch.uint8, device=dev)
    one = lambda t: (ctypes.c_void_p * 1)(t.data_ptr())
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.axvs_tl_loss_fwd(cfg, one(cls), one(masks), gt.data_ptr(), labels.data_ptr(), mv, cw.data_ptr(), match.data_ptr(), None,
                                    rand.data_ptr(), ntm.data_ptr(), losses.data_ptr(), rows.data_ptr(), cols.data_ptr(), cost.data_ptr(), None,
                                    saved.data_ptr(), ws.data_ptr(), ws.numel(), st), "axvs_tl_loss_fwd")
    g = torch.tensor(tc.upstream_weights(L), device=dev, dtype=torch.float32)
    dcls, dmasks = torch.empty_like(cls), torch.full_like(masks, float("nan"))
    _lib.check(lib.axvs_tl_loss_bwd(cfg, g.data_ptr(), one(cls), one(masks), gt.data_ptr(), mv, cw.data_ptr(), ntm.data_ptr(), saved.data_ptr(),
                                    one(dcls), one(dmasks), st), "axvs_tl_loss_bwd")
    torch.cuda.synchronize()
    assert torch.equal(rows[0].cpu(), r["rows"][0][0]) and torch.equal(cols[0].cpu(), r["cols"][0][0])
    assert torch.equal(rows[0].cpu(), fx.ref_pairs[0][0][0]) and torch.equal(cols[0].cpu(), fx.ref_pairs[0][0][1])
    ratios = dict(cost=tc.tensor_err(cost[0], r["cost"][0][0]) / yard["cost"],
                  losses=max(tc.scalar_err(losses[0, j], r["losses"][0, j]) for j in range(3)) / yard["losses"],
                  dcls=tc.tensor_err(dcls, r["dcls"][0]) / yard["dcls"], dmasks=tc.tensor_err(dmasks, r["dmasks"][0]) / yard["dmasks"])
    print("[tl_loss] hand_placed: " + ";  ".join(f"{q} {ratios[q]:.2f} x reference ({yard[q]:.3e})" for q in ratios))
    for q, v in ratios.items():
        assert v <= MARGIN, (q, v)


def test_autograd_reaches_the_cross_clip_head():
    """2 clips x 1 frame, Q = 5, 7 x 9: the losses of TubeLinkCrossClipHead's train() outputs back-propagate into the clip queries and
    the head's parameters"""
    import axial_vs_amd as ax
    import axvs_oracle as orc
    K, Cm, layers, B, Tc, Q, h, w = 4, 128, 2, 1, 2, 5, 7, 9
    mod = ax.TubeLinkCrossClipHead(num_classes=K, out_channels=Cm, num_cc_layers=layers)
    mod.load_state_dict(orc.random_weights({k: tuple(v.shape) for k, v in mod.state_dict().items()}, 31), strict=True)
    mod = mod.cuda().train()
    g = torch.Generator().manual_seed(32)
    cq = torch.randn(B, Tc, Q, 256, generator=g).cuda().requires_grad_(True)
    mf = torch.nn.functional.normalize(torch.randn(B, Tc, Cm, h, w, generator=g), dim=2).cuda()
    cls, masks = mod(cq, mf)
    assert len(cls) == layers and masks[0].shape == (B, Tc, Q, h, w) and cls[0].shape == (B, Q, K + 1)
    gt = torch.zeros(2, Tc, h, w, dtype=torch.uint8)
    gt[0, :, 1:4, 2:6] = 1
    gt[1, :, 3:7, 0:5] = 1
    crit = ax.TubeLinkSetCriterion(K, loss_cls=dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=2.0, class_weight=[1.0] * K + [0.1]),
                                   train_cfg=dict(num_points=64))
    losses = crit.loss(cls, masks, [torch.tensor([1, 3]).cuda()], [gt.cuda()], None, generator=torch.Generator(device="cuda").manual_seed(5))
    assert list(losses) == tc.loss_keys(layers)
    sum(losses.values()).backward()
    assert cq.grad is not None and bool(torch.isfinite(cq.grad).all()) and float(cq.grad.abs().max()) > 0
    for name, p in mod.named_parameters():
        if name.startswith(("cls_embed", "mask_embed")):
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, name


@pytest.mark.parametrize("kw, word", [(dict(Q=513), "Q=513"), (dict(P=16385), "num_points=16385"), (dict(P=64, over=1100.0), "S=70400"),
                                      (dict(T=1200), "T*h=8400"), (dict(M=513), "m_per_video[0]=513")])
def test_out_of_bounds_configurations_raise(kw, word):
    import axial_vs_amd as ax
    Q, P, T, M, over = kw.get("Q", 5), kw.get("P", 64), kw.get("T", 1), kw.get("M", 2), kw.get("over", 1.0)
    cls, masks = torch.zeros(1, 1, Q, 5, device="cuda"), torch.zeros(1, 1, T, Q, 7, 3, device="cuda")
    labels, gt = [torch.zeros(M, dtype=torch.int64, device="cuda")], [torch.zeros(M, T, 7, 3, dtype=torch.uint8, device="cuda")]
    coords = (torch.zeros(1, 1, P, 2, device="cuda"), torch.zeros(1, min(Q, M), int(P * over), 2, device="cuda"), torch.zeros(1, min(Q, M), P, 2, device="cuda"))
    with pytest.raises(RuntimeError, match=word.replace("[", r"\[").replace("]", r"\]").replace("*", r"\*")):
        ax.tube_link_losses(cls, masks, labels, gt, num_classes=4, class_weight=[1.0] * 5, num_points=P, oversample_ratio=over,
                            importance_sample_ratio=0.0, point_coords=coords)
    with pytest.raises(NotImplementedError, match="fp32"):
        ax.tube_link_losses(cls.half(), masks.half(), labels, gt, num_classes=4, class_weight=[1.0] * 5, num_points=64)
    with pytest.raises(NotImplementedError, match="bool, uint8 or fp32"):
        ax.tube_link_losses(cls[:, :, :5], masks[:, :, :1, :5], [labels[0][:2]], [gt[0][:2, :1].half()], num_classes=4, class_weight=[1.0] * 5, num_points=64)
