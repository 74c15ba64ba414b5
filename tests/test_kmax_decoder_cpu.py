"""CPU: the restatement of Video-kMaX's k-means query decoder (tests/kmax_decoder_cases.py) against fixtures of the reference's own
classes, the screening of the cases, the frame-crossing depthwise window, the module's state-dict names, and the argument errors of the
module and of the C-ABI (axvs_kmax_*), which are reported before any device work."""
import ctypes
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


def load_fixture(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    m = json.loads(bytes(z["meta"]).decode())
    case = kc.Case(m["name"], m["seed"], m["L"], m["K"], m["T"], tuple(tuple(s) for s in m["levels"]), tuple(m["pan"]), tuple(m["in_channels"]),
                   tuple(m["dec_layers"]), m["B"], m["mask_gain"])
    return case, m, z


@pytest.mark.parametrize("name", [c.name for c in kc.CASES])
def test_case_screening(name):
    """A condition on the stored seeds, not a measurement: the float32 restatement (free-running, and teacher-forced on the float64
    queries) takes the float64 restatement's cluster at every pixel of every layer, and no pixel's top-two margin lies within 8 x the
    float32 logit error.  The device tests compare index maps exactly and outputs end to end on that ground."""
    st = kc.study(kc.BY_NAME[name])
    for i, y in enumerate(st["layers"]):
        print(f"{name} layer {i}: flips {y['flips_tf']} / {y['flips_free']}, closest margin {float(y['margin'].min()):.2e}, "
              f"bands {y['band_tf']:.2e} / {y['band_free']:.2e}")
        assert y["flips_tf"] == 0 and y["flips_free"] == 0, i
        assert float(y["margin"].min()) > max(y["band_tf"], y["band_free"]), i
    assert kc.clean(st)


@pytest.mark.parametrize("fx", [c.name for c in kc.FIXTURES])
def test_restatement_reproduces_the_reference(fx):
    """The reference's own eval forward (fp32) against the float32 restatement on the same weights and inputs: every layer's index
    map equal, every output within 8 x the float32 restatement's own error against float64."""
    case, m, z = load_fixture(fx)
    assert case._replace(seed=0) == next(c for c in kc.FIXTURES if c.name == fx)._replace(seed=0)
    st = kc.study(case)
    assert m["keys"] == list(kc.param_shapes(case))
    for i, y in enumerate(st["layers"]):
        assert torch.equal(torch.from_numpy(z[f"index{i}"].astype(np.int64)), y["index"]), i
        assert y["flips_free"] == 0
    for k in ("pred_logits", "pred_mask_embeddings", "cluster_centers"):
        own = float((st["out32"][k].double() - st["out"][k]).abs().max())
        err = float((torch.from_numpy(z[k]) - st["out32"][k]).abs().max())
        print(f"{fx} {k}: reference vs float32 restatement {err:.3e}, float32 restatement vs float64 {own:.3e}")
        assert err <= 8 * own, k
    for k in ("pred_masks", "pixel_feature"):
        own = float((st["out32"][k].double() - st["out"][k]).abs().max())
        err = float((torch.from_numpy(z[k + "_row"]) - st["out32"][k][:, :, -1, 0]).abs().max())
        assert err <= 8 * own, k
        chk, t = z[k + "_checks"], st["out"][k]
        assert abs(chk[0] - float(t.sum())) <= 8 * own * t.numel() and abs(chk[2] - float(t.abs().max())) <= 8 * own, k


def test_depthwise_window_crosses_frame_boundaries():
    """Frames are stacked along the height before the predictor's 5 x 5 depthwise convolution: a change in the first row of frame 1
    changes `pixel_feature` in the last two rows of frame 0 (and not above them)."""
    case = kc.BY_NAME["f"]
    with torch.no_grad():
        params = kc.make_params(case)
        x, pan = kc.make_inputs(case)
        r = kc.Restatement(params, case, torch.float64)
        q = r.start()
        a = r.final(q, pan)["pixel_feature"]
        pan2 = pan.clone()
        pan2[1, :, 0, :] += 1.0                       # frame 1, first row
        b = r.final(q, pan2)["pixel_feature"]
    changed = (a != b).any(-1).any(1)[0]              # [T, H]
    H = case.pan[0]
    assert bool(changed[0, H - 2:].all()) and not bool(changed[0, :H - 2].any())
    assert bool(changed[1, :3].all()) and not bool(changed[1, 3:].any())


@pytest.mark.parametrize("name", ["a", "c"])
def test_state_dict_names(name):
    """The module carries the reference's own parameter and buffer names, in the reference's order (recorded in the fixtures from the
    reference's state_dict()), with the reference's shapes; a checkpoint with the training-only keys loads after the filter."""
    import axial_vs_amd as ax
    case = kc.BY_NAME[name]
    mod = ax.KMaXTransformerDecoder(case.dec_layers, case.in_channels, case.K, case.L, case.T, case.B > 1)
    sd = mod.state_dict()
    assert list(sd) == list(kc.param_shapes(case))
    assert {k: tuple(v.shape) for k, v in sd.items()} == dict(kc.param_shapes(case))
    ck = dict(kc.make_params(case))
    ck["_auxiliary_semantic_predictor.final_conv.conv.weight"] = torch.zeros(case.K + 1, 256, 1, 1)
    with pytest.raises(RuntimeError):
        mod.load_state_dict(ck, strict=True)
    mod.load_state_dict(ax.filter_training_keys(ck), strict=True)
    assert torch.equal(mod.state_dict()["_cluster_centers.weight"], ck["_cluster_centers.weight"])


def test_fixture_names_are_the_modules():
    import axial_vs_amd as ax
    for fx in kc.FIXTURES:
        case, m, _ = load_fixture(fx.name)
        mod = ax.KMaXTransformerDecoder(case.dec_layers, case.in_channels, case.K, case.L, case.T, case.B > 1)
        assert list(mod.state_dict()) == m["keys"]


def test_module_argument_errors():
    import axial_vs_amd as ax
    ok = dict(dec_layers=[2, 2, 2], in_channels=[2048, 1024, 512], num_classes=124, num_queries=128, num_clip_frames=2)
    ax.KMaXTransformerDecoder(**dict(ok, dec_layers=[1, 0, 0], in_channels=[32, 16, 16], num_queries=3, num_classes=1))
    for bad in (dict(num_queries=257), dict(num_queries=0), dict(num_classes=256), dict(in_channels=[2048, 1024, 520]), dict(in_channels=[4096, 16, 16]),
                dict(num_clip_frames=17), dict(dec_layers=[6, 6, 6]), dict(dec_layers=[0, 0, 0]), dict(dec_layers=[2, 2])):
        with pytest.raises(NotImplementedError):
            ax.KMaXTransformerDecoder(**dict(ok, **bad))


def test_train_mode_and_cpu_tensors_are_refused():
    import axial_vs_amd as ax
    case = kc.BY_NAME["c"]
    mod = ax.KMaXTransformerDecoder(case.dec_layers, case.in_channels, case.K, case.L, case.T, True)
    x, pan = kc.make_inputs(case)
    assert mod.training
    with pytest.raises(NotImplementedError):
        mod(x, pan)
    mod.eval()
    with pytest.raises(RuntimeError, match="GPU tensor"):
        mod(x, pan)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ax.kmax_decoder_forward(kc.make_params(case), x, pan, case.dec_layers, case.T, True)


def _cfg(case, **over):
    from axial_vs_amd.kmax_decoder import _cfg as mk
    cfg = mk(case.B, case.T, case.L, case.K + 1, case.dec_layers, case.in_channels, case.levels, (256,) + tuple(case.pan))
    for k, v in over.items():
        if isinstance(v, tuple):
            getattr(cfg, k)[v[0]] = v[1]
        else:
            setattr(cfg, k, v)
    return cfg


def test_abi_sizes_agree_with_the_parameter_order():
    """axvs_kmax_decoder_packed_bytes is the sum over axial_vs_amd/_params.py's slots (each rounded up to 256 bytes), and the folded
    tensors have the slots' shapes in the structs' order."""
    from axial_vs_amd import _lib, _params
    L = _lib.lib()
    for case in kc.CASES:
        chans = [case.in_channels[l] for l in kc.layer_levels(case)]
        assert L.axvs_kmax_decoder_packed_bytes(ctypes.byref(_cfg(case))) == _params.kmax_packed_bytes(case.L, case.K + 1, chans)
        assert L.axvs_kmax_decoder_workspace_bytes(ctypes.byref(_cfg(case))) > 0
        for i in range(len(chans)):
            assert L.axvs_kmax_stage_workspace_bytes(ctypes.byref(_cfg(case)), i, 0) > 0
            assert 0 < L.axvs_kmax_stage_workspace_bytes(ctypes.byref(_cfg(case)), i, 1) <= L.axvs_kmax_decoder_workspace_bytes(ctypes.byref(_cfg(case)))
    case = kc.BY_NAME["b"]
    sd = kc.make_params(case)
    assert [n for n, _ in _params.kmax_layer_shapes(64, 125)] == list(_lib.KMAX_LAYER_FIELDS)
    assert [n for n, _ in _params.kmax_head_shapes(100, 125)] == list(_lib.KMAX_HEAD_FIELDS)
    assert [tuple(t.shape) for t in _params.kmax_head_folded(sd)] == [s for _, s in _params.kmax_head_shapes(case.L, case.K + 1)]
    for i, l in enumerate(kc.layer_levels(case)):
        got = _params.kmax_layer_folded(sd, f"_kmax_transformer_layers.{i}.")
        assert [tuple(t.shape) for t in got] == [s for _, s in _params.kmax_layer_shapes(case.in_channels[l], case.K + 1)]
        assert all(t.dtype == torch.float64 for t in got)


def test_abi_bounds():
    """every bound of include/axvs.h's axvs_kmax_* section is refused with a message, before any device work"""
    from axial_vs_amd import _lib
    L = _lib.lib()
    case = kc.BY_NAME["a"]
    assert L.axvs_kmax_decoder_workspace_bytes(ctypes.byref(_cfg(case, L=1, K1=1))) > 0
    for over, word in ((dict(L=0), "queries"), (dict(L=257), "queries"), (dict(K1=257), "class"), (dict(K1=0), "class"), (dict(T=17), "frames"),
                       (dict(num_layers=0), "num_layers"), (dict(num_layers=17), "num_layers"), (dict(layer_level=(1, 3)), "level"),
                       (dict(in_channels=(1, 72)), "channels"), (dict(in_channels=(0, 4096)), "channels"), (dict(in_channels=(2, 0)), "channels"),
                       (dict(pan_channels=128), "256"), (dict(heads=4), "8"), (dict(base_filters=64), "128"), (dict(h=(0, 0)), "pixels"),
                       (dict(W=0), "pixels"), (dict(H=1 << 14), "H"), (dict(B=0), "clips")):
        cfg = _cfg(case, **over)
        assert L.axvs_kmax_decoder_packed_bytes(ctypes.byref(cfg)) == 0 and L.axvs_kmax_decoder_workspace_bytes(ctypes.byref(cfg)) == 0, over
        assert word in L.axvs_last_error().decode(), (over, L.axvs_last_error().decode())
        rc = L.axvs_kmax_decoder_fwd(ctypes.byref(cfg), None, None, None, None, None, None, None, None, None, None, 0, None)
        assert rc != 0, over
    cfg = _cfg(case)
    assert L.axvs_kmax_stage_workspace_bytes(ctypes.byref(cfg), 6, 0) == 0 and L.axvs_kmax_stage_workspace_bytes(ctypes.byref(cfg), -1, 1) == 0
    assert L.axvs_kmax_decoder_fwd(ctypes.byref(cfg), None, None, None, None, None, None, None, None, None, None, 0, None) != 0
    assert "null pointer" in L.axvs_last_error().decode()
    assert L.axvs_kmax_assign_fwd(ctypes.byref(cfg), None, 0, None, None, None, None, None, 0, None) != 0
    assert L.axvs_kmax_layer_fwd(ctypes.byref(cfg), None, 6, None, None, None, None, None, 0, None) != 0
    assert "layer" in L.axvs_last_error().decode()


def test_workspace_has_no_logits_term():
    """The memory condition, exactly: with both full-resolution outputs off, what a call allocates is its workspace (plus outputs of
    B*L rows), and the workspace's growth with the number of pixels of a level does not depend on L -- it holds no B*L*T*h*w term for any
    layer (the reference's logits, one-hot tensor and aux outputs are all of that size).  The cluster-sum slabs are capped at 64 chunks."""
    from axial_vs_amd import _lib
    L = _lib.lib()
    case = kc.BY_NAME["a"]

    def ws(Lq, h):
        cfg = _cfg(case, L=Lq, h=(2, h), want_masks=0, want_pixel_feature=0)
        return L.axvs_kmax_decoder_workspace_bytes(ctypes.byref(cfg))

    for h0, h1 in ((12, 24), (400, 800), (800, 1600)):          # below and above the chunk cap (T*h*w = 2*h*20 pixels)
        grow = [ws(Lq, h1) - ws(Lq, h0) for Lq in (16, 128, 256)]
        assert grow[0] == grow[1] == grow[2] > 0, (h0, h1, grow)
        # per pixel: gelu(x) C_l floats, three 256-channel rows, one 128-channel row, one index -- nothing else
        per_pixel = 4 * (case.in_channels[2] + 3 * 256 + 128) + 4
        assert abs(grow[0] - per_pixel * 2 * (h1 - h0) * 20) <= 8 * 256, (grow[0], per_pixel)
