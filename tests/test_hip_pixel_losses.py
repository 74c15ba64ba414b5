"""GPU: the sampled pixel losses of the within-clip criterion (axial_vs_amd.sampled_pixel_losses / MaXTronWCSetCriterion with
"pixels" and "aux_semantic") against the float64 restatement and the reference's sample sets, with the reference's own fp32 error as
the yardstick (tests/pixel_loss_cases.py).

Measured device error / reference error per fixture: profiles/pixel_losses_parity.txt."""
import pytest
import torch

import __graft_entry__ as ge
import pixel_loss_cases as pc

pytestmark = pytest.mark.gpu
MARGIN = pc.MARGIN
FOUR = ["labels", "masks", "pixels", "aux_semantic"]


@pytest.fixture(scope="module", autouse=True)
def built():
    ge.build()


def _call(out, targets, K, share, kp, ks, noise):
    import axial_vs_amd as ax
    return ax.sampled_pixel_losses(out, targets, K, share_final_matching=share, pixel_insdis_temperature=pc.TEMPERATURES[0],
                                   pixel_insdis_sample_k=kp, aux_semantic_temperature=pc.TEMPERATURES[1], aux_semantic_sample_k=ks,
                                   noise=noise, return_samples=True)


def _run(fx, weights):
    """forward, device-side weighted sum, backward -> (losses dict, samples, d pixel_feature per layer, d aux_semantic_pred)"""
    out = fx.outputs("cuda", requires_grad=True)
    losses, samples = _call(out, fx.targets_on("cuda"), fx.K, fx.share, fx.kp, fx.ks, fx.noise_on("cuda"))
    w = torch.tensor(weights, device="cuda")
    (torch.stack(list(losses.values())) * w).sum().backward()
    layers = [out] + list(out.get("aux_outputs", []))
    return losses, samples, [o["pixel_feature"].grad for o in layers], out["aux_semantic_pred"].grad


_runs = {}


def _shared_run(name):
    if name not in _runs:
        fx = pc.fixture(name)
        _runs[name] = _run(fx, pc.upstream_weights(fx.L + 1))
    return _runs[name]


def _device_sets(fx, samples):
    """rows of pc.row_plan: the L `pixels` rows, then the `aux_semantic` row -> [[int64 cpu index vector per video]]"""
    sp, ss = samples["pixels"].cpu().long(), samples["aux_semantic"].cpu().long()
    return [[sp[l, b] for b in range(fx.B)] for l in range(fx.L)] + [[ss[b] for b in range(fx.B)]]


@pytest.mark.parametrize("name", list(pc.CASES))
def test_sample_sets_equal_the_float64_and_the_reference_sets(name):
    fx = pc.fixture(name)
    _, samples, _, _ = _shared_run(name)
    got = _device_sets(fx, samples)
    for r, per in enumerate(fx.sets64()):
        for b, (idx, key, void, gap) in enumerate(per):
            assert got[r][b].numel() == (fx.kp if r < fx.L else fx.ks)
            assert torch.equal(got[r][b], idx), (r, b)                         # increasing pixel order, the float64 set
            assert torch.equal(got[r][b], fx.ref_samples[r][b]), (r, b)        # ... which is the reference's
            dev_key = (samples["keys_pixels"][r, b] if r < fx.L else samples["keys_aux_semantic"][b]).double().cpu()
            assert float((dev_key - key).abs().max()) < 0.02                   # fp32 at 1e5 resolves 0.0078; elsewhere a few 1e-7


@pytest.mark.parametrize("name", list(pc.CASES))
def test_losses_and_gradients_match_float64_within_eight_times_the_reference_error(name):
    fx = pc.fixture(name)
    weights = pc.upstream_weights(fx.L + 1)
    yl, yg = fx.yard()
    ref, rdf, rds = fx.restated(weights)
    losses, samples, df, ds = _shared_run(name)
    assert list(losses) == fx.keys
    el = max(pc.scalar_err(losses[k], ref[k]) for k in fx.keys)
    egf = max(pc.grad_err(df[l], rdf[l]) for l in range(fx.L))
    egs = pc.grad_err(ds, rds)
    print(f"[pixel_losses] {name}: losses {el:.3e} = {el / yl:.2f} x reference ({yl:.3e});  d pixel_feature {egf:.3e} = {egf / yg:.2f} x, "
          f"d aux_semantic_pred {egs:.3e} = {egs / yg:.2f} x reference ({yg:.3e})")
    assert el <= MARGIN * yl
    assert egf <= MARGIN * yg and egs <= MARGIN * yg


@pytest.mark.parametrize("name", list(pc.CASES))
def test_the_gradient_at_unsampled_pixels_is_exactly_zero(name):
    fx = pc.fixture(name)
    _, samples, df, ds = _shared_run(name)
    got = _device_sets(fx, samples)
    for l in range(fx.L):
        for b in range(fx.B):
            hit = torch.zeros(fx.P, dtype=torch.bool)
            hit[got[l][b]] = True
            assert float(df[l][b].flatten(1).cpu()[:, ~hit].abs().max() if (~hit).any() else 0.0) == 0.0
    for b in range(fx.B):
        hit = torch.zeros(fx.P, dtype=torch.bool)
        hit[got[fx.L][b]] = True
        assert float(ds[b].flatten(1).cpu()[:, ~hit].abs().max() if (~hit).any() else 0.0) == 0.0


def test_exact_zeros():
    """a video without objects is all void: its instance-discrimination term and gradient are exactly 0, its semantic term is not; a
    semantic map that is entirely ignored gives exactly 0 and a zero gradient; k = 0 gives exactly 0"""
    fx = pc.fixture("g25_pixel_losses_M0")
    losses, _, df, ds = _shared_run(fx.name)
    assert all(float(df[l][1].abs().max()) == 0.0 and float(df[l][0].abs().max()) > 0.0 for l in range(fx.L))
    assert float(ds[1].abs().max()) > 0.0
    fx = pc.fixture("g25_pixel_losses_semignore")
    losses, _, df, ds = _shared_run(fx.name)
    assert float(losses["loss_aux_semantic"]) == 0.0 and float(ds.abs().max()) == 0.0 and float(losses["loss_pixel_insdis"]) > 0.0
    fx = pc.fixture("g25_pixel_losses_k63")
    out = fx.outputs("cuda", requires_grad=True)
    losses, samples = _call(out, fx.targets_on("cuda"), fx.K, fx.share, 0, 0, fx.noise_on("cuda"))
    assert list(losses) == fx.keys and all(float(v) == 0.0 for v in losses.values())
    assert samples["pixels"].shape[-1] == 0 and samples["aux_semantic"].shape[-1] == 0
    sum(losses.values()).backward()
    assert float(out["pixel_feature"].grad.abs().max()) == 0.0 and float(out["aux_semantic_pred"].grad.abs().max()) == 0.0


def test_no_video_has_an_object():
    """the second video of the M0 fixture alone: no targets at all reach the library (no pairs, no concatenated targets); every pixel is
    void, the instance-discrimination loss is exactly 0 and the semantic loss is the restatement's"""
    fx = pc.fixture("g25_pixel_losses_M0")
    out = fx.outputs("cuda", requires_grad=True)
    one = lambda d: {k: v[1:2].detach().clone().requires_grad_(v.requires_grad) for k, v in d.items() if k != "aux_outputs"}
    sub = dict(one(out), aux_outputs=[one(o) for o in out["aux_outputs"]])
    up, us = fx.noise_on("cuda")
    losses, samples = _call(sub, fx.targets_on("cuda")[1:], fx.K, fx.share, fx.kp, fx.ks, (up[:, 1:2].contiguous(), us[1:2].contiguous()))
    assert list(losses) == fx.keys
    assert all(float(losses[k]) == 0.0 for k in fx.keys if "insdis" in k)
    x = fx.layers[0]["aux_semantic_pred"][1].double().flatten(1)
    ref = pc.semantic64(x, fx.targets[1]["semantic_masks"].reshape(-1), torch.arange(fx.P), fx.K)
    assert pc.scalar_err(losses["loss_aux_semantic"], ref) < pc.fp32_bound(fx.K, fx.ks)
    sum(losses.values()).backward()
    assert float(sub["pixel_feature"].grad.abs().max()) == 0.0 and float(sub["aux_semantic_pred"].grad.abs().max()) > 0.0


@pytest.mark.parametrize("name", ["g25_pixel_losses_P1100", "g25_pixel_losses_k65_own"])
def test_two_runs_are_bit_equal(name):
    fx = pc.fixture(name)
    a, b = _shared_run(name), _run(fx, pc.upstream_weights(fx.L + 1))
    assert all(torch.equal(a[0][k], b[0][k]) for k in fx.keys)
    assert torch.equal(a[1]["pixels"], b[1]["pixels"]) and torch.equal(a[1]["aux_semantic"], b[1]["aux_semantic"])
    assert all(torch.equal(x, y) for x, y in zip(a[2], b[2])) and torch.equal(a[3], b[3])


def test_k_above_P_and_bad_shapes_raise():
    fx = pc.fixture("g25_pixel_losses_k1")
    tg, noise = fx.targets_on("cuda"), fx.noise_on("cuda")
    with pytest.raises(RuntimeError, match="out of range"):
        _call(fx.outputs("cuda"), tg, fx.K, fx.share, fx.P + 1, 1, noise)
    with pytest.raises(RuntimeError, match="8193"):
        _call(fx.outputs("cuda"), tg, fx.K, fx.share, 1, 8193, noise)
    out = fx.outputs("cuda")
    out["pixel_feature"] = out["pixel_feature"][:, :3]
    with pytest.raises(RuntimeError, match="3 channels"):
        _call(out, tg, fx.K, fx.share, 1, 1, noise)
    with pytest.raises(RuntimeError, match="noise"):
        _call(fx.outputs("cuda"), tg, fx.K, fx.share, 1, 1, (noise[0][:, :, :-1], noise[1]))


def test_void_pixels_are_taken_lowest_index_first_when_the_objects_are_smaller_than_k():
    """UNSCREENED: 10 non-void pixels, k = 40.  Every non-void pixel is sampled, the other 30 are void pixels whose fp32 keys sit near
    -99999 (resolution 0.0078) and tie: among equal keys the lower pixel index is kept.  The losses are compared with the restatement
    on the device's own sample sets within the format-derived bound of pixel_loss_cases.fp32_bound (the reference's choice among
    tied keys is unspecified, so it gives no yardstick here)."""
    import axial_vs_amd as ax
    name, case = "sparse_k40", pc.UNSCREENED_CASES["sparse_k40"]
    N, Ms, K, T, H, W, L, share, kind, C, kp, ks, semkind = case
    B, P = len(Ms), T * H * W
    layers, targets = pc.make_case(case, 0)
    torch.manual_seed(4)
    u_pix, u_sem = ax.draw_sampling_noise(L, B, P, True, True, "cpu")
    dev = lambda d: {k: v.cuda() for k, v in d.items()}
    ls = [dev(o) for o in layers]
    for o in ls:
        o["pixel_feature"].requires_grad_(True)
    ls[0]["aux_semantic_pred"].requires_grad_(True)
    out = dict(ls[0], aux_outputs=ls[1:])
    tg = [dev(t) for t in targets]
    losses, samples = _call(out, tg, K, bool(share), kp, ks, (u_pix.cuda(), u_sem.cuda()))
    pairs = [[(r.cpu(), c.cpu()) for r, c in ax.match_layers(out, tg)[0][0]]]
    nonvoid = [t["masks"].flatten(1).any(0) for t in targets]
    keys = [samples["keys_pixels"][l].cpu() for l in range(L)] + [samples["keys_aux_semantic"].cpu()]
    sets = [[samples["pixels"][l, b].cpu().long() for b in range(B)] for l in range(L)] + [[samples["aux_semantic"][b].cpu().long() for b in range(B)]]
    ties = 0
    for r in range(L + 1):
        for b in range(B):
            idx, key = sets[r][b], keys[r][b]
            assert idx.numel() == 40 and bool((idx[1:] > idx[:-1]).all())
            sel = torch.zeros(P, dtype=torch.bool)
            sel[idx] = True
            assert bool(sel[nonvoid[b]].all()) and int((sel & ~nonvoid[b]).sum()) == 40 - int(nonvoid[b].sum())
            thr = key[idx].min()
            assert bool(sel[key > thr].all()) and not bool(sel[key < thr].any())
            eq = (key == thr).nonzero().flatten()
            n = int(sel[eq].sum())
            assert torch.equal(eq[sel[eq]], eq[:n])                              # equal keys: the lower indices
            ties += int(eq.numel() > n)
    print(f"[pixel_losses] {name}: {ties} of {(L + 1) * B} rows cut through a group of equal keys")
    l64 = [{k: v.detach().double().cpu().requires_grad_(k in ("pixel_feature", "aux_semantic_pred")) for k, v in o.items()} for o in ls]
    ref = pc.losses64(l64, targets, pairs, N, K, bool(share), sets)
    sum(ref.values()).backward()
    sum(losses.values()).backward()
    bound = pc.fp32_bound(max(C, K), max(kp, ks))
    el = max(pc.scalar_err(losses[k], ref[k]) for k in ref)
    eg = max([pc.grad_err(ls[l]["pixel_feature"].grad, l64[l]["pixel_feature"].grad) for l in range(L)] +
             [pc.grad_err(ls[0]["aux_semantic_pred"].grad, l64[0]["aux_semantic_pred"].grad)])
    print(f"[pixel_losses] {name}: losses {el:.3e}, gradients {eg:.3e} against the restatement on the device's sets (bound {bound:.3e})")
    assert list(losses) == list(ref) and el < bound and eg < bound


def test_the_within_clip_criterion_returns_the_reference_keys_and_the_same_labels_and_masks_losses():
    """all four losses: the reference's keys in its order (per prediction: the losses in list order, aux_semantic for the final one
    only); the labels / masks entries are bit-equal to what the class gives for ["labels", "masks"]; a seeded call repeats bit for bit;
    the backward reaches every prediction's pixel_feature and aux_semantic_pred"""
    import axial_vs_amd as ax
    fx = pc.fixture("g25_pixel_losses_k63")
    tg = fx.targets_on("cuda")
    kw = dict(process_semantic=True, pixel_insdis_temperature=pc.TEMPERATURES[0], pixel_insdis_sample_k=fx.kp,
              aux_semantic_temperature=pc.TEMPERATURES[1], aux_semantic_sample_k=fx.ks)
    four = ax.MaXTronWCSetCriterion(fx.K, ax.VideoHungarianMatcher(), {}, 0.1, FOUR, fx.share, **kw)
    two = ax.MaXTronWCSetCriterion(fx.K, ax.VideoHungarianMatcher(), {}, 0.1, ["labels", "masks"], fx.share, **kw)
    out = fx.outputs("cuda", requires_grad=True)
    for o in [out] + out["aux_outputs"]:
        o["pred_masks"].requires_grad_(True)
        o["pred_logits"].requires_grad_(True)
    torch.manual_seed(11)
    a = four(out, tg)
    assert list(a) == ["loss_ce", "loss_mask", "loss_dice", "loss_pixel_insdis", "loss_aux_semantic",
                       "loss_ce_0", "loss_mask_0", "loss_dice_0", "loss_pixel_insdis_0"]
    assert all(v.dim() == 0 and v.dtype == torch.float32 and v.is_cuda for v in a.values())
    b = two(fx.outputs("cuda"), tg)
    assert all(torch.equal(a[k], b[k]) for k in b) and len(b) == 6
    torch.manual_seed(11)
    c = four(fx.outputs("cuda"), tg)
    assert all(torch.equal(a[k], c[k]) for k in a)
    torch.manual_seed(12)
    d = four(fx.outputs("cuda"), tg)
    assert not torch.equal(a["loss_pixel_insdis"], d["loss_pixel_insdis"])          # another draw, other samples
    sum(a.values()).backward()
    for o in [out] + out["aux_outputs"]:
        assert float(o["pixel_feature"].grad.abs().max()) > 0.0 and float(o["pred_masks"].grad.abs().max()) > 0.0
    assert float(out["aux_semantic_pred"].grad.abs().max()) > 0.0
    with pytest.raises(RuntimeError, match="process_semantic"):
        ax.MaXTronWCSetCriterion(fx.K, ax.VideoHungarianMatcher(), {}, 0.1, FOUR, fx.share)(fx.outputs("cuda"), tg)
