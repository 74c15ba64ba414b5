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


ALL_CASES = {**cc.CASES, **cc.EDGE_CASES}
_runs = {}


def _shared_run(name):
    """one device run per fixture with the upstream weights of cc.upstream_weights, shared by the tests that only read it"""
    if name not in _runs:
        fx = cc.fixture(name)
        _runs[name] = _run(fx, cc.upstream_weights(fx.L))
    return _runs[name]


def _split_over_workgroups(fx):
    """from the library's size query: every problem's pixel range goes to at least two workgroups (a workgroup's partial sums are
    4 N + 2 floats)"""
    from axial_vs_amd import _lib
    return _lib.lib().axvs_set_criterion_workspace_bytes(fx.L, fx.B, fx.N, fx.K + 1, fx.P) >= 2 * fx.L * fx.B * (4 * fx.N + 2) * 4


def _run(fx, weights):
    """forward, device-side weighted sum, backward -> (losses dict, d pred_masks per layer, d pred_logits per layer)"""
    out = fx.outputs("cuda", requires_grad=True)
    losses = _criterion(fx)(out, fx.targets_on("cuda"))
    w = torch.tensor(weights, device="cuda")
    (torch.stack(list(losses.values())) * w).sum().backward()
    layers = [out] + list(out.get("aux_outputs", []))
    return losses, [o["pred_masks"].grad for o in layers], [o["pred_logits"].grad for o in layers]


@pytest.mark.parametrize("name", list(cc.CASES) + list(cc.EDGE_CASES))
def test_losses_and_gradients_match_float64_within_eight_times_the_reference_error(name):
    """N = 1: d pred_masks is zero in exact arithmetic (the softmax over one query is constant) and in the float64 restatement, so no
    relative measure applies.  Every factor of the device's expression (probability, clamped weight, 0.75 / (N B)) is at most 1 and the
    upstream weights are below 2, so a cancelled fp32 expression leaves a few units of 2^-24: the largest magnitude must be at most 2^-20."""
    fx = cc.fixture(name)
    weights = cc.upstream_weights(fx.L)
    yl, yg = fx.yard()
    ref, rdm, rdl = fx.restated(weights)
    losses, dm, dl = _shared_run(name)
    assert list(losses) == cc.loss_keys(fx.L)
    el = max(cc.scalar_err(losses[k], ref.reshape(-1)[i]) for i, k in enumerate(cc.loss_keys(fx.L)))
    if fx.N == 1:
        egm = max(float(dm[l].abs().max()) for l in range(fx.L))
        print(f"[criterion] {name}: largest |d pred_masks| {egm:.3e}")
        assert egm <= 2.0 ** -20
        egm = 0.0
    else:
        egm = max(cc.grad_err(dm[l], rdm[l]) for l in range(fx.L))
    egl = max(cc.grad_err(dl[l], rdl[l]) for l in range(fx.L))
    print(f"[criterion] {name}: losses {el:.3e} = {el / yl:.2f} x reference ({yl:.3e});  d pred_masks {egm:.3e} = {egm / yg:.2f} x, "
          f"d pred_logits {egl:.3e} = {egl / yg:.2f} x reference ({yg:.3e})")
    assert el <= MARGIN * yl
    assert egm <= MARGIN * yg and egl <= MARGIN * yg


@pytest.mark.parametrize("name", list(cc.EDGE_CASES))
def test_device_pairs_equal_the_stored_ones(name):
    """the criterion uses the matcher's pairs but never shows them: match_layers on the same inputs gives the fixture's rows / cols"""
    import axial_vs_amd as ax
    fx = cc.fixture(name)
    got = ax.match_layers(fx.outputs("cuda"), fx.targets_on("cuda"), masking_void_pixel=fx.masking)
    assert len(got) == fx.L
    for j, per_video in enumerate(fx.pairs):                  # (one stored matching when it is shared: the final prediction's)
        ind = got[j][0]
        assert len(ind) == fx.B
        for b, (rows, cols) in enumerate(per_video):
            assert len(rows) == min(fx.N, fx.meta["M"][b])
            assert torch.equal(ind[b][0].cpu(), rows) and torch.equal(ind[b][1].cpu(), cols), (j, b)


@pytest.mark.parametrize("name", cc.SPLIT)
def test_split_cases_are_split_over_workgroups(name):
    """a change of the plan that gives one of these problems a single workgroup fails here instead of silently emptying the case.
    P = 300 is 5 tiles, which no plan with workgroups of 2 or more tiles divides evenly; P = 581 is 10 tiles (4, 4 and 2 today)."""
    fx = cc.fixture(name)
    assert _split_over_workgroups(fx)
    assert ((fx.P + 63) // 64) in (5, 10)


@pytest.mark.parametrize("name", [n for n, c in ALL_CASES.items() if c[8]])
def test_gradient_at_void_pixels_is_exactly_zero(name):
    """under masking_void_pixel, d pred_masks is exactly 0 (not small) at every pixel the float64 restatement calls void, and over the
    whole slice of a video without objects: an error relative to the largest entry would let dust or a stale value pass"""
    fx = cc.fixture(name)
    _, dm, _ = _shared_run(name)
    void = cc.void_pixels(fx)
    seen = 0
    for l in range(fx.L):
        j = 0 if fx.share else l
        for b in range(fx.B):
            v = void[j][b]
            seen += int(v.sum())
            assert torch.count_nonzero(dm[l][b].flatten(1)[:, v.cuda()]) == 0, (l, b)
            if fx.meta["M"][b] == 0:
                assert bool(v.all()) and torch.count_nonzero(dm[l][b]) == 0, (l, b)
    assert seen > 0 or fx.N == 1          # (the one pixel of the N = 1 case belongs to its object)


@pytest.mark.parametrize("name", [cc.BIG, cc.RAGGED] + cc.ANY_SPLIT)
def test_second_run_is_bit_equal(name):
    fx = cc.fixture(name)
    if name == cc.BIG:          # the 128-query problem spans several workgroups: its partial sums are added in workgroup order
        from axial_vs_amd import _lib
        L = _lib.lib()
        one = L.axvs_set_criterion_workspace_bytes(1, 1, fx.N, fx.K + 1, 64)
        assert L.axvs_set_criterion_workspace_bytes(fx.L, fx.B, fx.N, fx.K + 1, fx.P) >= 2 * fx.L * fx.B * one
    if name in cc.ANY_SPLIT:    # the any-size kernels' partials, from several workgroups with a short last range
        assert fx.N > 128 and _split_over_workgroups(fx)
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


# ---- input forms: each bit-equal to the contiguous fp32 run of the same values, which the parity test checks against float64 ----------
FORMS = "g19_criterion_N7_M9-2_L2_share_mv0"          # B = 2, two layers, shared matching


def _forms_run(fx, preds, targets, leaves):
    """preds: per layer {"pred_masks", "pred_logits"} as handed to the criterion; leaves: the tensors whose .grad is returned"""
    out = dict(preds[0], aux_outputs=list(preds[1:]))
    losses = _criterion(fx)(out, targets)
    w = torch.tensor(cc.upstream_weights(fx.L), device="cuda")
    (torch.stack(list(losses.values())) * w).sum().backward()
    return losses, [t.grad for t in leaves]


def _fp32_run(fx, values=None, targets=None):
    """the contiguous fp32 run on `values` (default: the fixture's) -> (losses, d pred_masks per layer + d pred_logits per layer)"""
    values = fx.layers if values is None else values
    preds = [{k: v.cuda().float().contiguous().requires_grad_(True) for k, v in o.items()} for o in values]
    return _forms_run(fx, preds, fx.targets_on("cuda") if targets is None else targets,
                      [o["pred_masks"] for o in preds] + [o["pred_logits"] for o in preds])


def _same_losses(a, b):
    return list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_sixteen_bit_predictions_are_scored_as_fp32_and_get_gradients_in_their_dtype(dtype):
    """the fixture values are fp16-representable, so the fp16 run sees the fp32 run's numbers; the bf16 run is compared with an fp32 run
    on the bf16-rounded values.  Losses bit-equal, gradients in the input dtype and equal to the fp32 run's gradients rounded to it."""
    fx = cc.fixture(FORMS)
    rounded = [{k: v.to(dtype).float() for k, v in o.items()} for o in fx.layers]
    if dtype == torch.float16:
        assert all(torch.equal(r[k], o[k]) for r, o in zip(rounded, fx.layers) for k in o)
    else:
        assert not torch.equal(rounded[0]["pred_masks"], fx.layers[0]["pred_masks"])
    ref_losses, ref_grads = _fp32_run(fx, rounded)
    preds = [{k: v.cuda().to(dtype).requires_grad_(True) for k, v in o.items()} for o in fx.layers]
    losses, grads = _forms_run(fx, preds, fx.targets_on("cuda"), [o["pred_masks"] for o in preds] + [o["pred_logits"] for o in preds])
    assert all(v.dtype == torch.float32 for v in losses.values()) and _same_losses(losses, ref_losses)
    for g, r in zip(grads, ref_grads):
        assert g.dtype == dtype and g.shape == r.shape and torch.equal(g, r.to(dtype))
    assert all(float(r.abs().max()) > 0.0 for r in ref_grads)


def test_non_contiguous_predictions_give_the_same_bits_in_their_leaves_shapes():
    """pred_masks as the models hand it over: a permuted view of a [B, T, H, W, N] leaf; pred_logits: a slice of a wider leaf"""
    fx = cc.fixture(FORMS)
    ref_losses, ref_grads = _fp32_run(fx)
    K1 = fx.K + 1
    g = torch.Generator().manual_seed(7)
    mleaves = [o["pred_masks"].permute(0, 2, 3, 4, 1).contiguous().cuda().requires_grad_(True) for o in fx.layers]
    lleaves = []
    for o in fx.layers:
        wide = torch.randn(fx.B, fx.N, K1 + 3, generator=g)
        wide[..., :K1] = o["pred_logits"]
        lleaves.append(wide.cuda().requires_grad_(True))
    preds = [{"pred_masks": m.permute(0, 4, 1, 2, 3), "pred_logits": w[..., :K1]} for m, w in zip(mleaves, lleaves)]
    assert all(not o["pred_masks"].is_contiguous() and not o["pred_logits"].is_contiguous() for o in preds)
    assert all(o["pred_masks"].shape == f["pred_masks"].shape for o, f in zip(preds, fx.layers))
    losses, grads = _forms_run(fx, preds, fx.targets_on("cuda"), mleaves + lleaves)
    assert _same_losses(losses, ref_losses)
    for l in range(fx.L):
        assert grads[l].shape == mleaves[l].shape and torch.equal(grads[l], ref_grads[l].permute(0, 2, 3, 4, 1))
        gl = grads[fx.L + l]
        assert gl.shape == lleaves[l].shape and torch.equal(gl[..., :K1], ref_grads[fx.L + l]) and torch.count_nonzero(gl[..., K1:]) == 0


@pytest.mark.parametrize("form", ["uint8", "sliced_bool", "int32_labels", "bool_and_float"])
def test_target_forms_give_the_same_bits(form):
    """uint8 masks, a non-contiguous bool mask (a slice along W of a wider one whose other columns are set) and int32 labels against the
    bool / int64 run; a batch of a float video and a bool video (the `x.float()` branch of _cat_targets) against the all-float run"""
    fx = cc.fixture(FORMS)
    assert fx.B == 2 and fx.kind == "bool"
    tg = fx.targets_on("cuda")
    base = tg
    if form == "uint8":
        other = [{"labels": t["labels"], "masks": t["masks"].to(torch.uint8)} for t in tg]
    elif form == "sliced_bool":
        W = fx.meta["W"]
        wide = [torch.ones(t["masks"].shape[:-1] + (W + 3,), dtype=torch.bool, device="cuda") for t in tg]
        for w, t in zip(wide, tg):
            w[..., :W] = t["masks"]
        other = [{"labels": t["labels"], "masks": w[..., :W]} for w, t in zip(wide, tg)]
        assert all(not o["masks"].is_contiguous() and torch.equal(o["masks"], t["masks"]) for o, t in zip(other, tg))
    elif form == "int32_labels":
        other = [{"labels": t["labels"].to(torch.int32), "masks": t["masks"]} for t in tg]
    else:
        base = [{"labels": t["labels"], "masks": t["masks"].float()} for t in tg]
        other = [base[0], tg[1]]
        assert other[0]["masks"].dtype == torch.float32 and other[1]["masks"].dtype == torch.bool
    ref_losses, ref_grads = _fp32_run(fx, targets=base)
    losses, grads = _fp32_run(fx, targets=other)
    assert _same_losses(losses, ref_losses)
    assert all(torch.equal(g, r) for g, r in zip(grads, ref_grads))
    assert float(ref_losses["loss_mask"]) > 0.0 and float(ref_losses["loss_dice_0"]) > 0.0


def test_blank_targets_give_exact_zeros():
    """objects whose masks are all zero (criterion_cases.UNSCREENED_CASES; no fixture: every similarity is 0, every assignment ties and
    none passes the generator's stability screen).  Under masking every pixel is void: loss_mask and loss_dice are exactly 0.0 and
    d pred_masks is exactly 0 whatever the matching (max(count, 1) in the forward, gm in the backward).  loss_ce and d pred_logits do
    depend on the matching (a matched query's weight is the clamped 1e-5 and its label the object's), and the optimum is unique neither
    with the masking matcher nor with an `mv = 0` one (the similarities are 0 either way), so the comparison with one float64 optimum
    is left out.  Instead the pairs the device's own matcher returns are checked to be a complete assignment, and loss_ce / d pred_logits
    are compared with criterion64 on THOSE pairs at the format-derived bound (cc.fp32_bound)."""
    import axial_vs_amd as ax
    (case,) = cc.UNSCREENED_CASES.values()
    N, Ms, K, T, H, W, L, share, mv, kind = case
    layers, targets = cc.make_case(case, 0)
    dev = [{k: v.cuda().requires_grad_(True) for k, v in o.items()} for o in layers]
    tg = [{k: v.cuda() for k, v in t.items()} for t in targets]
    out = dict(dev[0], aux_outputs=dev[1:])
    ind = ax.match_layers({k: v.detach() for k, v in dev[0].items()}, tg, masking_void_pixel=True)[0][0]
    pairs = [[(r.cpu(), c.cpu()) for r, c in ind]]
    for (rows, cols), M in zip(pairs[0], Ms):
        k = min(N, M)
        assert len(rows) == len(cols) == k and len(set(rows.tolist())) == k and len(set(cols.tolist())) == k
        assert 0 <= int(rows.min()) and int(rows.max()) < N and 0 <= int(cols.min()) and int(cols.max()) < M
    crit = ax.MaXTronCCSetCriterion(K, ax.VideoHungarianMatcher(masking_void_pixel=True), {}, 0.1, ["labels", "masks"], True, masking_void_pixel=True)
    got = crit(out, tg)
    w = torch.tensor(cc.upstream_weights(L), dtype=torch.float64)
    (torch.stack(list(got.values())) * w.float().cuda()).sum().backward()
    ls = [{k: v.double().requires_grad_(True) for k, v in o.items()} for o in layers]
    ref = cc.criterion64(ls, targets, pairs, K, True, True)
    (ref.reshape(-1) * w).sum().backward()
    bound = cc.fp32_bound(N, T * H * W, K)
    for l in range(L):
        sfx = "" if l == 0 else f"_{l - 1}"
        assert float(got["loss_mask" + sfx]) == 0.0 and float(got["loss_dice" + sfx]) == 0.0
        assert torch.count_nonzero(dev[l]["pred_masks"].grad) == 0
        assert float(ref[l, 0]) > 0.0 and cc.scalar_err(got["loss_ce" + sfx], ref[l, 0]) <= bound
        assert cc.grad_err(dev[l]["pred_logits"].grad, ls[l]["pred_logits"].grad) <= bound


def test_batch_without_objects_gives_empty_indices_and_errors_are_still_reported():
    """no video has an object (a training clip without objects): the matcher returns indices of length 0 per video and the criterion
    its losses, without an error from the library; a refused call afterwards in the same process still raises with the library's text"""
    import axial_vs_amd as ax
    fx = cc.fixture("g19_criterion_N6_M0-0_L2_share_mv1")
    assert fx.meta["M"] == [0, 0]
    out, tg = fx.outputs("cuda"), fx.targets_on("cuda")
    ind, dice, cls = ax.VideoHungarianMatcher(masking_void_pixel=True)(out, tg)
    assert len(ind) == len(dice) == len(cls) == fx.B
    for b in range(fx.B):
        assert ind[b][0].shape == ind[b][1].shape == dice[b].shape == cls[b].shape == (0,)
        assert ind[b][0].dtype == ind[b][1].dtype == torch.int64 and ind[b][0].is_cuda
    assert all(m.shape == (fx.N, 0) for per_video in ax.matcher_costs(out, tg) for m in per_video)
    losses = _criterion(fx)(out, tg)
    assert float(losses["loss_mask"]) == 0.0 and float(losses["loss_dice_0"]) == 0.0 and float(losses["loss_ce"]) > 0.0
    wide = {"pred_masks": torch.zeros(1, 513, 1, 8, 8, device="cuda"), "pred_logits": torch.zeros(1, 513, 5, device="cuda")}
    one = [{"labels": torch.zeros(2, dtype=torch.int64, device="cuda"), "masks": torch.ones(2, 1, 8, 8, dtype=torch.bool, device="cuda")}]
    with pytest.raises(RuntimeError, match="512"):
        ax.set_criterion_losses(wide, one, 4)
    none = [{"labels": torch.zeros(0, dtype=torch.int64, device="cuda"), "masks": torch.zeros(0, 1, 8, 8, dtype=torch.bool, device="cuda")}]
    with pytest.raises(RuntimeError, match="512"):
        ax.set_criterion_losses(wide, none, 4)
