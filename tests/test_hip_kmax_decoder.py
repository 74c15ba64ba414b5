"""GPU: Video-kMaX's k-means query decoder (axial_vs_amd.KMaXTransformerDecoder, axvs_kmax_*) against the float64 restatement of
tests/kmax_decoder_cases.py.  Bounds: index maps are compared outside a band of 8 x the float32 restatement's own logit error against
float64 (on the screened cases no pixel lies inside it: every pixel is compared), numbers within 8 x the float32 restatement's own
error (9 x against fixtures of the reference, whose fp32 run carries 1 x itself).  The float64 and float32 restatements of a case run
once (kmax_decoder_cases.study) and are shared."""
import json
import os

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
import kmax_decoder_cases as kc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="session", autouse=True)
def built():
    ge.build()


def make_decoder(case, params=None):
    import axial_vs_amd as ax
    dec = ax.KMaXTransformerDecoder(case.dec_layers, case.in_channels, case.K, case.L, case.T, case.B > 1)
    dec.load_state_dict(kc.make_params(case) if params is None else params, strict=True)
    return dec.cuda().eval()


_DEVICE = {}
_FREE = {}


@pytest.fixture(scope="module", autouse=True)
def release_device_state():
    """a decoder is ~80 MB of parameters and packed weights: this module's shared device state is dropped when its tests are done, so
    that tests which measure peak device memory see what they saw before"""
    yield
    _DEVICE.clear()
    _FREE.clear()
    if torch.cuda.is_available():
        torch.cuda.empty_cache()


def on_device(case):
    """(study, decoder, features, panoptic features) of a case, on the device once"""
    if case.name not in _DEVICE:
        st = kc.study(case)
        _DEVICE[case.name] = (st, make_decoder(case, st["params"]), [t.cuda() for t in st["x"]], st["pan"].cuda())
    return _DEVICE[case.name]


def rows(q):
    """the restatement's queries [B, 256, L] -> the device's rows [B, L, 256], fp32"""
    return q.transpose(1, 2).float().contiguous().cuda()


def outside_band(y, band):
    return y["margin"] > band


ALL = [c.name for c in kc.CASES]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL)
def test_assign_teacher_forced(name):
    """The assignment of every layer on the float64 chain's queries: the float64 cluster at every pixel whose top-two margin is outside
    the band (every pixel, on the screened cases), class logits within 8 x the float32 restatement's error."""
    st, dec, x, _ = on_device(kc.BY_NAME[name])
    for i, y in enumerate(st["layers"]):
        idx, cls = dec.assign(rows(y["q_in"]), x[y["level"]], i)
        idx = idx.cpu().long()
        assert int(idx.min()) >= 0 and int(idx.max()) < st["case"].L
        diff = idx != y["index"]
        keep = outside_band(y, y["band_tf"])
        err = float((cls.double().cpu() - y["class_logits"]).abs().max())
        print(f"{name} layer {i}: {int(diff.sum())} of {diff.numel()} pixels differ, {int((~keep).sum())} inside the band {y['band_tf']:.2e}; "
              f"class logits {err:.2e}, bound {y['tol_cls']:.2e}")
        assert bool(keep.all()), i                         # the screening's promise
        assert not bool((diff & keep).any()), i
        assert err <= y["tol_cls"], i


def hand_maps(case, S):
    L = case.L
    p = torch.arange(case.B * S, dtype=torch.int64).view(case.B, S)
    spread = (p % L)
    last = torch.full_like(p, L - 1)
    no0 = 1 + p % (L - 1)                                   # cluster 0 empty
    return dict(spread=spread, last=last, no0=no0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["a", "b", "c", "e"])
def test_layer_with_given_index_maps(name):
    """A layer given its index map, against float64 within 8 x the float32 restatement's error under the same map: the float64
    chain's own map and three maps built by hand -- p % L (every cluster used), all pixels in cluster L - 1 (the longest sum), and
    cluster 0 empty, whose row then takes the sum-free path: it does not depend on the pixel values at all, bit for bit."""
    st, dec, x, _ = on_device(kc.BY_NAME[name])
    case = st["case"]
    for i, y in enumerate(st["layers"]):
        l = y["level"]
        S = case.T * case.levels[l][0] * case.levels[l][1]
        maps = dict(own=y["index"], **hand_maps(case, S))
        stacked = kc.stack(st["x"][l], case.B)
        for tag, m in maps.items():
            with torch.no_grad():
                want, _, _ = st["r64"].layer(i, stacked.double(), y["q_in"], index=m)
                own, _, _ = st["r32"].layer(i, stacked, y["q_in"].float(), index=m)
            tol = 8 * float((own.double() - want).abs().max())
            got = dec.layer(rows(y["q_in"]), x[l], m.int().cuda(), i)
            err = float((got.double().cpu() - want.transpose(1, 2)).abs().max())
            print(f"{name} layer {i} map {tag}: {err:.2e}, bound {tol:.2e}")
            assert err <= tol, (i, tag)
            if tag == "no0":
                other = dec.layer(rows(y["q_in"]), x[l] * 2.0 + 1.0, m.int().cuda(), i)
                assert torch.equal(other[:, 0], got[:, 0]), i
                assert not torch.equal(other[:, 1], got[:, 1]), i


@pytest.mark.gpu
def test_layer_at_the_chunk_cap():
    """16928 pixels in one clip: past 64 x 256, where the cluster sums' chunks grow instead of their number (66 chunks of 256 would be
    needed; the split is 53 of 320, the last one partial), with levels that no layer reads.  A layer given three hand-built maps
    against float64, within 8 x the float32 restatement's error under the same map."""
    case = kc.Case("cap", 900, 8, 3, 2, ((2, 2), (2, 2), (92, 92)), (4, 4), (16, 16, 16), (0, 0, 1), 1, 0.1)
    with torch.no_grad():
        params = kc.make_params(case)
        x, _ = kc.make_inputs(case)
        r64, r32 = kc.Restatement(params, case, torch.float64), kc.Restatement(params, case, torch.float32)
        dec = make_decoder(case, params)
        stacked, q = kc.stack(x[2], 1), r64.start()
        S = case.T * 92 * 92
        for tag, m in hand_maps(case, S).items():
            want, _, _ = r64.layer(0, stacked.double(), q, index=m)
            own, _, _ = r32.layer(0, stacked, q.float(), index=m)
            tol = 8 * float((own.double() - want).abs().max())
            got = dec.layer(rows(q), x[2].cuda(), m.int().cuda(), 0)
            err = float((got.double().cpu() - want.transpose(1, 2)).abs().max())
            print(f"cap map {tag}: {err:.2e}, bound {tol:.2e}")
            assert err <= tol, tag


def free_run(case):
    if case.name not in _FREE:
        st, dec, x, pan = on_device(case)
        _FREE[case.name] = dec(x, pan, return_index_maps=True)
    return _FREE[case.name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL)
def test_free_run(name):
    """The whole decoder: every layer's index map equals float64's, all five outputs within 8 x the float32 restatement's own error
    (max-norm per tensor); the ratios go to profiles/kmax_decoder_parity.txt."""
    case = kc.BY_NAME[name]
    st = kc.study(case)
    out = free_run(case)
    assert out["aux_outputs"] == []
    for i, y in enumerate(st["layers"]):
        assert torch.equal(out["index_maps"][i].cpu().long(), y["index"]), i
    lines, bad = [], []
    for k in kc.OUTPUTS:
        assert out[k].shape == st["out"][k].shape, k
        err = float((out[k].double().cpu() - st["out"][k]).abs().max())
        own = st["tol"][k] / 8
        lines.append(f"{name:>18} {k:>22}: device {err:.3e}  float32 restatement {own:.3e}  ratio {err / own:.2f}")
        if err > st["tol"][k]:
            bad.append(k)
    print("\n".join(lines))
    if os.environ.get("AXVS_WRITE_PARITY"):
        with open(os.environ["AXVS_WRITE_PARITY"], "a") as f:
            f.write("\n".join(lines) + "\n")
    assert not bad, bad


def load_fixture(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    m = json.loads(bytes(z["meta"]).decode())
    case = kc.Case(m["name"], m["seed"], m["L"], m["K"], m["T"], tuple(tuple(s) for s in m["levels"]), tuple(m["pan"]), tuple(m["in_channels"]),
                   tuple(m["dec_layers"]), m["B"], m["mask_gain"])
    return case, z


@pytest.mark.gpu
@pytest.mark.parametrize("fx", [c.name for c in kc.FIXTURES])
def test_reference_fixture(fx):
    """The reference's own fp32 forward: index maps equal, outputs within 9 x the float32 restatement's error (8 x ours + 1 x the reference's own)."""
    case, z = load_fixture(fx)
    st = kc.study(case)
    out = free_run(case)
    for i in range(len(st["layers"])):
        assert torch.equal(out["index_maps"][i].cpu().long(), torch.from_numpy(z[f"index{i}"].astype(np.int64))), i
    for k in ("pred_logits", "pred_mask_embeddings", "cluster_centers"):
        err = float((out[k].cpu() - torch.from_numpy(z[k])).abs().max())
        print(f"{fx} {k}: {err:.3e}, bound {9 * st['tol'][k] / 8:.3e}")
        assert err <= 9 * st["tol"][k] / 8, k
    for k in ("pred_masks", "pixel_feature"):
        err = float((out[k][:, :, -1, 0].cpu() - torch.from_numpy(z[k + "_row"])).abs().max())
        assert err <= 9 * st["tol"][k] / 8, k


@pytest.mark.gpu
def test_stacked_clips_equal_single_clips():
    """Case c: three clips through cross_clip_training in one call, and each clip alone -- equal bits in every output and index map."""
    case = kc.BY_NAME["c"]
    st, dec, x, pan = on_device(case)
    whole = free_run(case)
    single = make_decoder(case._replace(B=1), st["params"])
    assert not single._cross_clip_training
    T = case.T
    for b in range(case.B):
        one = single([t[b * T:(b + 1) * T] for t in x], pan[b * T:(b + 1) * T], return_index_maps=True)
        for k in kc.OUTPUTS:
            assert torch.equal(one[k][0], whole[k][b]), (b, k)
        for a, w in zip(one["index_maps"], whole["index_maps"]):
            assert torch.equal(a[0], w[b]), b


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["a", "b"])
def test_two_runs_give_equal_bits(name):
    case = kc.BY_NAME[name]
    st, dec, x, pan = on_device(case)
    first = free_run(case)
    again = dec(x, pan, return_index_maps=True)
    for k in kc.OUTPUTS:
        assert torch.equal(first[k], again[k]), k
    for a, b in zip(first["index_maps"], again["index_maps"]):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_side_stream():
    case = kc.BY_NAME["f"]
    st, dec, x, pan = on_device(case)
    want = free_run(case)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got = dec(x, pan)
    s.synchronize()
    for k in kc.OUTPUTS:
        assert torch.equal(got[k], want[k]), k


@pytest.mark.gpu
def test_output_flags():
    """return_pred_masks / return_pixel_feature switch the two full-resolution outputs off; the rest is unchanged, bit for bit."""
    case = kc.BY_NAME["g"]
    st, dec, x, pan = on_device(case)
    want = free_run(case)
    try:
        for masks, pix in ((False, True), (True, False), (False, False)):
            dec.return_pred_masks, dec.return_pixel_feature = masks, pix
            got = dec(x, pan)
            assert (got["pred_masks"] is None) == (not masks) and (got["pixel_feature"] is None) == (not pix)
            for k in kc.OUTPUTS:
                if got[k] is not None:
                    assert torch.equal(got[k], want[k]), (masks, pix, k)
    finally:
        dec.return_pred_masks = dec.return_pixel_feature = True


@pytest.mark.gpu
def test_module_equals_functional_and_repacks():
    """load_state_dict of a reference-named state dict, then forward: the functional call on the same tensors gives the same bits; a
    parameter or running statistic changed in place is seen by the next forward."""
    import axial_vs_amd as ax
    case = kc.BY_NAME["f"]
    st, dec, x, pan = on_device(case)
    want = free_run(case)
    params = {k: v.cuda() for k, v in st["params"].items()}
    params["_auxiliary_semantic_predictor.0.conv.weight"] = torch.zeros(1, device="cuda")
    got = ax.kmax_decoder_forward(params, x, pan, case.dec_layers, case.T, case.B > 1)
    for k in kc.OUTPUTS:
        assert torch.equal(got[k], want[k]), k
    mod = make_decoder(case, st["params"])
    with torch.no_grad():
        mod._predictor._pixel_space_mask_batch_norm.running_mean.add_(0.5)
    params["_predictor._pixel_space_mask_batch_norm.running_mean"] = params["_predictor._pixel_space_mask_batch_norm.running_mean"] + 0.5
    a, b = mod(x, pan), ax.kmax_decoder_forward(params, x, pan, case.dec_layers, case.T, case.B > 1)
    assert torch.equal(a["pred_masks"], b["pred_masks"]) and not torch.equal(a["pred_masks"], want["pred_masks"])
    with torch.no_grad():
        mod._predictor._pixel_space_mask_batch_norm.running_mean.sub_(0.5)
        first = mod(x, pan)["pred_masks"]
        mod._predictor._pixel_space_mask_batch_norm.weight.mul_(2.0)
        assert not torch.equal(mod(x, pan)["pred_masks"], first)


@pytest.mark.gpu
def test_cpu_tensors_are_refused():
    case = kc.BY_NAME["c"]
    st, dec, x, pan = on_device(case)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        dec([t.cpu() for t in x], pan)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        dec(x, pan.cpu())
    y = st["layers"][0]
    with pytest.raises(RuntimeError):
        dec.layer(rows(y["q_in"]), x[0], y["index"].int(), 0)          # a CPU index map
