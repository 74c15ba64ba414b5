"""GPU: the set criterion's losses and gradients (axial_vs_amd.set_criterion_losses / MaXTronCCSetCriterion) against the float64
restatement, with the reference's own fp32 error as the yardstick (tests/criterion_cases.py).

Measured device error / reference error per fixture: profiles/criterion_parity.txt."""
import pytest
import torch

import __graft_entry__ as ge
import criterion_cases as cc

pytestmark = pytest.mark.gpu
MARGIN = 8.0


@pytest.fixture(scope="module", autouse=True)
def built():
    ge.build()


def _criterion(fx):
    import axial_vs_amd as ax
    return ax.MaXTronCCSetCriterion(fx.K, ax.VideoHungarianMatcher(masking_void_pixel=fx.masking), {}, 0.1, ["labels", "masks"], fx.share,
                                    masking_void_pixel=fx.masking)


def _run(fx, weights):
    """forward, device-side weighted sum, backward -> (losses dict, d pred_masks per layer, d pred_logits per layer)"""
    out = fx.outputs("cuda", requires_grad=True)
    losses = _criterion(fx)(out, fx.targets_on("cuda"))
    w = torch.tensor(weights, device="cuda")
    (torch.stack(list(losses.values())) * w).sum().backward()
    layers = [out] + list(out.get("aux_outputs", []))
    return losses, [o["pred_masks"].grad for o in layers], [o["pred_logits"].grad for o in layers]


@pytest.mark.parametrize("name", list(cc.CASES))
def test_losses_and_gradients_match_float64_within_eight_times_the_reference_error(name):
    fx = cc.fixture(name)
    weights = cc.upstream_weights(fx.L)
    yl, yg = fx.yard()
    ref, rdm, rdl = fx.restated(weights)
    losses, dm, dl = _run(fx, weights)
    assert list(losses) == cc.loss_keys(fx.L)
    el = max(cc.scalar_err(losses[k], ref.reshape(-1)[i]) for i, k in enumerate(cc.loss_keys(fx.L)))
    egm = max(cc.grad_err(dm[l], rdm[l]) for l in range(fx.L))
    egl = max(cc.grad_err(dl[l], rdl[l]) for l in range(fx.L))
    print(f"[criterion] {name}: losses {el:.3e} = {el / yl:.2f} x reference ({yl:.3e});  d pred_masks {egm:.3e} = {egm / yg:.2f} x, "
          f"d pred_logits {egl:.3e} = {egl / yg:.2f} x reference ({yg:.3e})")
    assert el <= MARGIN * yl
    assert egm <= MARGIN * yg and egl <= MARGIN * yg


@pytest.mark.parametrize("name", [cc.BIG, cc.RAGGED])
def test_second_run_is_bit_equal(name):
    fx = cc.fixture(name)
    if name == cc.BIG:          # the 128-query problem spans several workgroups: its partial sums are added in workgroup order
        from axial_vs_amd import _lib
        L = _lib.lib()
        one = L.axvs_set_criterion_workspace_bytes(1, 1, fx.N, fx.K + 1, 64)
        assert L.axvs_set_criterion_workspace_bytes(fx.L, fx.B, fx.N, fx.K + 1, fx.P) >= 2 * fx.L * fx.B * one
    weights = cc.upstream_weights(fx.L)
    a, b = _run(fx, weights), _run(fx, weights)
    assert all(torch.equal(a[0][k], b[0][k]) for k in a[0])
    assert all(torch.equal(x, y) for x, y in zip(a[1] + a[2], b[1] + b[2]))


def test_no_host_synchronisation():
    fx = cc.fixture(cc.RAGGED)
    weights = cc.upstream_weights(fx.L)
    _run(fx, weights)                      # (first call: allocator, workspace, module loading)
    out, tg, crit = fx.outputs("cuda", requires_grad=True), fx.targets_on("cuda"), _criterion(fx)
    w = torch.tensor(weights, device="cuda")
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        losses = crit(out, tg)
        (torch.stack(list(losses.values())) * w).sum().backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert out["pred_masks"].grad is not None and out["aux_outputs"][0]["pred_logits"].grad is not None


def test_clip_outputs_select_the_matched_prediction():
    """matching on clip_outputs, losses on outputs (cc_criterion.py:423-432): equal to the restatement with that matching, and different
    from the criterion without clip_outputs"""
    import axial_vs_amd as ax
    from scipy.optimize import linear_sum_assignment  # noqa: F401  (the restatement's matcher)
    import matcher_cases as mc
    fx, other = cc.fixture("g19_criterion_N16_M5-0_L3_share_mv1"), cc.fixture("g19_criterion_N16_M5-0_L3_share_mv0")
    clip = {"pred_masks": fx.layers[1]["pred_masks"].flip(1), "pred_logits": fx.layers[1]["pred_logits"].flip(1)}
    pairs = [[mc.restate(clip["pred_masks"][b], clip["pred_logits"][b], t["masks"], t["labels"], True)[3:] if t["labels"].numel() else
              (torch.zeros(0, dtype=torch.int64),) * 2 for b, t in enumerate(fx.targets)]]
    assert not torch.equal(pairs[0][0][0], fx.pairs[0][0][0])
    ls = [{k: v.double() for k, v in o.items()} for o in fx.layers]
    ref = cc.criterion64(ls, fx.targets, pairs, fx.K, True, True, matched={k: v.double() for k, v in clip.items()})
    crit = _criterion(fx)
    got = crit(fx.outputs("cuda"), fx.targets_on("cuda"), {k: v.cuda() for k, v in clip.items()})
    plain = crit(fx.outputs("cuda"), fx.targets_on("cuda"))
    yl = max(fx.yard()[0], other.yard()[0])
    for i, k in enumerate(cc.loss_keys(fx.L)):
        assert cc.scalar_err(got[k], ref.reshape(-1)[i]) <= MARGIN * yl, k
    assert float(got["loss_dice"]) != float(plain["loss_dice"])
    wc = ax.MaXTronWCSetCriterion(fx.K, None, {}, 0.1, ["labels", "masks"], True)(fx.outputs("cuda"), fx.targets_on("cuda"))
    assert all(torch.equal(wc[k], plain[k]) for k in plain)
    only = ax.MaXTronCCSetCriterion(fx.K, None, {}, 0.1, ["masks"], True)(fx.outputs("cuda"), fx.targets_on("cuda"))
    assert list(only) == [k for k in cc.loss_keys(fx.L) if not k.startswith("loss_ce")]


def test_gradient_of_pred_masks_is_skipped_when_not_required():
    import axial_vs_amd as ax
    fx = cc.fixture("g19_criterion_N100_M1_L1_share_mv1")
    out = fx.outputs("cuda")
    out["pred_logits"].requires_grad_(True)
    losses = ax.set_criterion_losses(out, fx.targets_on("cuda"), fx.K, fx.masking, fx.share)
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    sum(losses.values()).backward()
    assert out["pred_masks"].grad is None and out["pred_logits"].grad is not None
    assert torch.cuda.max_memory_allocated() - before < out["pred_masks"].numel() * 4       # no d pred_masks buffer was made
    _, _, rdl = fx.restated()
    assert cc.grad_err(out["pred_logits"].grad, rdl[0]) <= MARGIN * fx.yard()[1]


def test_more_than_512_queries_raise():
    import axial_vs_amd as ax
    out = {"pred_masks": torch.zeros(1, 513, 1, 8, 8, device="cuda"), "pred_logits": torch.zeros(1, 513, 5, device="cuda")}
    tg = [{"labels": torch.zeros(2, dtype=torch.int64, device="cuda"), "masks": torch.ones(2, 1, 8, 8, dtype=torch.bool, device="cuda")}]
    with pytest.raises(RuntimeError, match="512"):
        ax.set_criterion_losses(out, tg, 4)


def test_more_than_128_queries_take_the_any_size_kernels():
    """N = 160 > 128 runs criterion_fwd_any_kernel / criterion_bwd_any_kernel.  No reference fixture has this size: the bound is the
    format-derived one of the CPU test (criterion_cases.fp32_bound), which every fixture's reference error meets with room."""
    import axial_vs_amd as ax
    import matcher_cases as mc
    case = (160, (9, 3), 6, 1, 10, 13, 2, 0, 1, "bool")
    N, Ms, K, T, H, W, L, share, mv, kind = case
    layers, targets = cc.make_case(case, 0)
    pairs = [[mc.restate(o["pred_masks"][b], o["pred_logits"][b], t["masks"], t["labels"], True)[3:] for b, t in enumerate(targets)] for o in layers]
    ls = [{k: v.double().requires_grad_(True) for k, v in o.items()} for o in layers]
    ref = cc.criterion64(ls, targets, pairs, K, True, False)
    w = torch.tensor(cc.upstream_weights(L), dtype=torch.float64)
    (ref.reshape(-1) * w).sum().backward()
    dev = [{k: v.cuda().requires_grad_(True) for k, v in o.items()} for o in layers]
    got = ax.set_criterion_losses(dict(dev[0], aux_outputs=dev[1:]), [{k: v.cuda() for k, v in t.items()} for t in targets], K, True, False)
    (torch.stack(list(got.values())) * w.float().cuda()).sum().backward()
    bound = cc.fp32_bound(N, T * H * W, K)
    for i, k in enumerate(cc.loss_keys(L)):
        assert cc.scalar_err(got[k], ref.reshape(-1)[i]) <= bound, k
    for l in range(L):
        assert cc.grad_err(dev[l]["pred_masks"].grad, ls[l]["pred_masks"].grad) <= bound
        assert cc.grad_err(dev[l]["pred_logits"].grad, ls[l]["pred_logits"].grad) <= bound


def test_losses_can_be_scaled_in_place_as_the_models_do():
    """maxtron_cc_model.py:315-319: `losses[k] *= self.criterion.weight_dict[k]`, then the sum is backpropagated"""
    fx = cc.fixture("g19_criterion_N16_M5-0_L3_share_mv1")
    weights = cc.upstream_weights(fx.L)
    out = fx.outputs("cuda", requires_grad=True)
    losses = _criterion(fx)(out, fx.targets_on("cuda"))
    for k, w in zip(list(losses), weights):
        losses[k] *= w
    sum(losses.values()).backward()
    _, rdm, _ = fx.restated(weights)
    assert cc.grad_err(out["pred_masks"].grad, rdm[0]) <= MARGIN * fx.yard()[1]
