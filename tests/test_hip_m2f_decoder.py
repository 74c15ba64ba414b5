"""GPU: Tube-Link's per-clip masked-attention query decoder (axial_vs_amd.TubeLinkClipDecoder, axvs_m2f_*) against the float64
restatement of tests/m2f_decoder_cases.py.  Bounds: attention-mask bits are compared outside a band of 8 x the fp32 restatement's own
logit error against float64, numbers within 8 x the fp32 restatement's own error (9 x against fixtures of the reference, whose fp32
run carries 1 x itself).  The float64 and fp32 restatements of a case run once (m2f_decoder_cases.study) and are shared."""
import json
import os

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
import m2f_decoder_cases as mc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ORDER = ("cross_attn", "norm", "self_attn", "norm", "ffn", "norm")


@pytest.fixture(scope="session", autouse=True)
def built():
    ge.build()


def decoder_cfg(layers, **layer_kw):
    lay = dict(type="DetrTransformerDecoderLayer",
               attn_cfgs=dict(type="MultiheadAttention", embed_dims=256, num_heads=8, attn_drop=0.0, proj_drop=0.0, dropout_layer=None, batch_first=False),
               ffn_cfgs=dict(embed_dims=256, feedforward_channels=2048, num_fcs=2, act_cfg=dict(type="ReLU", inplace=True), ffn_drop=0.0,
                             dropout_layer=None, add_identity=True),
               feedforward_channels=2048, operation_order=ORDER)
    lay.update(layer_kw)
    return dict(type="DetrTransformerDecoder", return_intermediate=True, num_layers=layers, transformerlayers=lay, init_cfg=None)


def make_decoder(case, params=None):
    import axial_vs_amd as ax
    dec = ax.TubeLinkClipDecoder(case.Q, case.K, feat_channels=256, out_channels=256, transformer_decoder=decoder_cfg(case.layers),
                                 positional_encoding=dict(type="SinePositionalEncoding3D", num_feats=128, normalize=True), num_transformer_feat_level=3)
    dec.load_state_dict(mc.make_params(case) if params is None else params, strict=True)
    return dec.cuda()


_DEVICE = {}


def on_device(name):
    """(study, decoder, mask features, memories) of a case, on the device once"""
    if name not in _DEVICE:
        st = mc.study(mc.BY_NAME[name])
        _DEVICE[name] = (st, make_decoder(st["case"], st["params"]), st["mf"].cuda(), [m.cuda() for m in st["mems"]])
    return _DEVICE[name]


def unpack(bits, S):
    from axial_vs_amd.clip_decoder import unpack_mask_bits
    return unpack_mask_bits(bits, S).cpu()


ALL = [c.name for c in mc.CASES]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL)
def test_mask_head_teacher_forced(name):
    """One mask head on the float64 chain's state: every bit outside the band equals float64's, the flags are equal, bits past the
    row's end are zero."""
    st, dec, mf, _ = on_device(name)
    case = st["case"]
    for i, l in enumerate(st["layers"]):
        lv, S = i % 3, mc.keys_of(case, i % 3)
        bits, flags = dec.attention_mask(l["x_in"].transpose(0, 1).float().cuda(), mf, case.levels[lv], lv)
        got = unpack(bits, S)
        diff = got != l["masked"]
        print(f"{name} layer {i}: {int(diff.sum())} of {diff.numel()} bits differ, band {l['band_tf']:.2e}")
        assert not bool((diff & (l["logits"].abs() > l["band_tf"])).any()), i
        open_any = (~got).any(-1)                      # the flag belongs to the bits the device wrote
        assert torch.equal(flags.cpu() != 0, open_any), i
        settled = (l["logits"].abs() > l["band_tf"]).all(-1)
        assert torch.equal((flags.cpu() != 0)[settled], (~l["masked"]).any(-1)[settled]), i
        W = bits.shape[-1]
        assert W == (S + 31) // 32
        if S % 32:
            assert int((bits[..., -1].cpu().to(torch.int64) & 0xFFFFFFFF).bitwise_right_shift(S % 32).abs().max()) == 0, i


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL)
def test_layer_teacher_forced(name):
    """One layer on the float64 chain's state with float64's bits: within 8 x the fp32 restatement's own error."""
    from axial_vs_amd.clip_decoder import pack_mask_bits
    st, dec, _, mems = on_device(name)
    for i, l in enumerate(st["layers"]):
        bits = pack_mask_bits(l["masked"]).cuda()
        flags = (~l["masked"].all(-1)).int().cuda()
        out = dec.layer(l["x_in"].transpose(0, 1).float().cuda(), mems[i % 3], bits, flags, i)
        err = float((out.double().cpu().transpose(0, 1) - l["x_out"]).abs().max())
        print(f"m2f layer parity: case {name} layer {i}: |device - float64| {err:.3e} = {8 * err / l['tol_layer']:.2f} x the fp32 restatement's")
        assert err <= l["tol_layer"], i


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL)
def test_decoder_free_running(name):
    """The whole decoder: no bit outside the free-running band differs (on the cases screened for it, no bit at all), and the queries
    and the last layer's predictions are within 8 x the fp32 free-running restatement's error."""
    st, dec, mf, mems = on_device(name)
    case = st["case"]
    q, cls, mp, lm = dec(mf, mems, return_predictions=True, return_masks=True)
    assert q.shape == (case.Q, case.N, 256) and cls.shape == (case.N, case.Q, case.K + 1) and mp.shape == (case.N, case.T, case.Q) + case.hw
    for i, (bits, flags) in enumerate(lm):
        l = st["layers"][i]
        got = unpack(bits, mc.keys_of(case, i % 3))
        diff = got != l["masked"]
        assert not bool((diff & (l["logits"].abs() > l["band_free"])).any()), i
        if name in mc.NO_FLIP:
            assert not bool(diff.any()), i
            assert torch.equal(flags.cpu() != 0, (~l["masked"]).any(-1)), i
    for what, got, ref, tol in (("query_feat", q, st["out"], st["tol_out"]), ("cls_pred", cls, st["cls"], st["tol_cls"]),
                                ("mask_pred", mp, st["mask_pred"], st["tol_mask"])):
        err = float((got.double().cpu() - ref).abs().max())
        print(f"m2f decoder parity: case {name} {what}: |device - float64| {err:.3e} = {8 * err / tol:.2f} x the fp32 restatement's")
        if name in mc.NO_FLIP:
            assert err <= tol, what
    q2 = dec(mf, mems)
    assert torch.equal(q2, q)              # the predictions and the debug output change nothing


@pytest.mark.gpu
@pytest.mark.parametrize("fx", [c.name for c in mc.FIXTURES])
def test_fixtures_of_the_reference(fx):
    """The reference's own forward (fp32): its attention-mask bits outside the band, its queries within 9 x the fp32 restatement's error
    (8 x for the device against float64 plus 1 x for the reference itself)."""
    z = np.load(os.path.join(GOLDEN, fx + ".npz"))
    m = json.loads(bytes(z["meta"]).decode())
    case = mc.Case(m["name"], m["seed"], m["N"], m["Q"], m["T"], tuple(m["hw"]), tuple(tuple(s) for s in m["levels"]), m["layers"], m["K"], m["boost"])
    with torch.no_grad():
        params, (mf, mems) = mc.make_params(case), mc.make_inputs(case)
        rec64, out64 = mc.Restatement(params, mf, mems, torch.float64, case.layers).run()
        rec32, out32 = mc.Restatement(params, mf, mems, torch.float32, case.layers).run()
    dec = make_decoder(case, params)
    assert sorted(dec.state_dict().keys()) == sorted(m["keys"])
    q, lm = dec(mf.cuda(), [x.cuda() for x in mems], return_masks=True)
    for i, (bits, flags) in enumerate(lm):
        S = mc.keys_of(case, i % 3)
        ref = torch.from_numpy(np.unpackbits(z[f"mask{i}"], axis=-1, bitorder="little")[..., :S].astype(bool))      # after the all-masked rule
        got = unpack(bits, S)
        got[flags.cpu() == 0] = False
        band = 9 * float((rec32[i]["logits"].double() - rec64[i]["logits"]).abs().max())
        assert not bool(((got != ref) & (rec64[i]["logits"].abs() > band)).any()), i
    own = float((out32.double() - out64).abs().max())
    err = float((q.double().cpu() - torch.from_numpy(z["query_feat"]).double().transpose(0, 1)).abs().max())
    print(f"m2f decoder parity: {fx}: |device - reference| {err:.3e} = {err / own:.2f} x the fp32 restatement's error")
    assert err <= 9 * own


@pytest.mark.gpu
def test_stacked_clips_equal_single_clips_bit_for_bit():
    st, dec, mf, mems = on_device("d")
    q = dec(mf, mems)
    for n in range(st["case"].N):
        one = dec(mf[n:n + 1], [m[n:n + 1] for m in mems])
        assert torch.equal(one[:, 0], q[:, n]), n


@pytest.mark.gpu
def test_two_runs_give_equal_bits():
    _, dec, mf, mems = on_device("e")
    a = dec(mf, mems, return_predictions=True, return_masks=True)
    b = dec(mf, mems, return_predictions=True, return_masks=True)
    for x, y in zip(a[:3], b[:3]):
        assert torch.equal(x, y)
    for (b0, f0), (b1, f1) in zip(a[3], b[3]):
        assert torch.equal(b0, b1) and torch.equal(f0, f1)


@pytest.mark.gpu
def test_side_stream():
    _, dec, mf, mems = on_device("c")
    want = dec(mf, mems)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = dec(mf, mems)
    side.synchronize()
    assert torch.equal(got, want)


def _scipy_match(tgt, cur):
    """TLCC:1038-1050 as written there (torch CPU + SciPy)"""
    from scipy.optimize import linear_sum_assignment
    cur = cur / cur.norm(dim=1)[:, None]
    tgt = tgt / tgt.norm(dim=1)[:, None]
    return torch.as_tensor(linear_sum_assignment((1.0 * (1 - torch.mm(cur, tgt.transpose(0, 1)))).transpose(0, 1))[1])


@pytest.mark.gpu
def test_tube_link_clip_queries():
    """Three clips of two videos: the stacked call equals the composition built by hand -- one decoder call per clip (checked against
    float64 above), SciPy's assignment on the device's own embeddings, the gather -- and feeds TubeLinkCrossClipHead."""
    import axial_vs_amd as ax
    case = mc.BY_NAME["f"]._replace(boost=0.0)
    dec = make_decoder(case, mc.make_params(case))
    B, Tc = case.N, 3
    clips = []
    for c in range(Tc):
        mf, mems = mc.make_inputs(case, case.seed + 10 * c)
        clips.append((mf.cuda(), [m.cuda() for m in mems]))
    got = ax.tube_link_clip_queries(dec, clips)
    assert got.shape == (B, Tc, case.Q, 256)
    per_clip = [dec(mf, mems).transpose(0, 1).cpu() for mf, mems in clips]          # [B,Q,C] each
    want = []
    for b in range(B):
        rows = [per_clip[0][b]]
        for c in range(1, Tc):
            idx = _scipy_match(rows[-1], per_clip[c][b])
            assert sorted(idx.tolist()) == list(range(case.Q))
            rows.append(per_clip[c][b][idx])
        want.append(torch.stack(rows))
    assert torch.equal(got.cpu(), torch.stack(want))
    head = ax.TubeLinkCrossClipHead(num_classes=case.K, num_cc_layers=1).cuda().eval()
    mask_features = torch.cat([c[0] for c in clips], dim=1)
    cls_a, masks_a = head(got, mask_features)
    cls_b, masks_b = head(torch.stack(want).cuda(), mask_features)
    assert cls_a[-1].shape == (B, case.Q, case.K + 1) and masks_a[-1].shape == (B, Tc * case.T, case.Q) + case.hw
    assert torch.equal(cls_a[-1], cls_b[-1]) and torch.equal(masks_a[-1], masks_b[-1]) and bool(torch.isfinite(masks_a[-1]).all())


def test_state_dict_keys_are_the_heads_own():
    """the key list a checkpoint of the head fills with strict=False: the one stored with the fixture of the reference's own module"""
    import axial_vs_amd as ax
    fx = mc.FIXTURES[0]
    m = json.loads(bytes(np.load(os.path.join(GOLDEN, fx.name + ".npz"))["meta"]).decode())
    dec = ax.TubeLinkClipDecoder(fx.Q, fx.K, transformer_decoder=decoder_cfg(fx.layers))
    assert sorted(dec.state_dict().keys()) == sorted(m["keys"])
    assert not dec.train().training          # frozen and in eval() in the head, whatever its mode


@pytest.mark.parametrize("kw", [
    dict(transformer_decoder=decoder_cfg(9, operation_order=("self_attn", "norm", "cross_attn", "norm", "ffn", "norm"))),
    dict(transformer_decoder=decoder_cfg(9, operation_order=("norm", "cross_attn", "norm", "self_attn", "norm", "ffn"))),       # pre-norm
    dict(transformer_decoder=decoder_cfg(9, attn_cfgs=dict(embed_dims=256, num_heads=8, attn_drop=0.1))),
    dict(transformer_decoder=decoder_cfg(9, ffn_cfgs=dict(embed_dims=256, feedforward_channels=2048, ffn_drop=0.1))),
    dict(transformer_decoder=decoder_cfg(9, attn_cfgs=dict(embed_dims=256, num_heads=4))),
    dict(transformer_decoder=decoder_cfg(9, ffn_cfgs=dict(embed_dims=256, feedforward_channels=1024))),
    dict(transformer_decoder=decoder_cfg(17)),
    dict(feat_channels=128), dict(num_transformer_feat_level=4), dict(enforce_decoder_input_project=True),
    dict(positional_encoding=dict(type="SinePositionalEncoding3D", num_feats=64, normalize=True)),
])
def test_unsupported_configurations_raise_at_construction(kw):
    import axial_vs_amd as ax
    with pytest.raises(NotImplementedError):
        ax.TubeLinkClipDecoder(100, 40, **kw)


def test_cpu_tensors_are_refused():
    import axial_vs_amd as ax
    case = mc.BY_NAME["c"]
    dec = ax.TubeLinkClipDecoder(case.Q, case.K, transformer_decoder=decoder_cfg(case.layers))
    mf, mems = mc.make_inputs(case)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        dec(mf, mems)
