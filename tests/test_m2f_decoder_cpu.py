"""CPU: the restatement of Tube-Link's per-clip query decoder (tests/m2f_decoder_cases.py) against fixtures of the reference's own
classes, the invariant the device path rests on (the resize commutes with the mask einsum), the screening of the cases, and the
argument errors of the C-ABI (axvs_m2f_*), which are reported before any device work."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
import m2f_decoder_cases as mc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="session", autouse=True)
def built():
    ge.build()


def load_fixture(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    m = json.loads(bytes(z["meta"]).decode())
    case = mc.Case(m["name"], m["seed"], m["N"], m["Q"], m["T"], tuple(m["hw"]), tuple(tuple(s) for s in m["levels"]), m["layers"], m["K"], m["boost"])
    masks = [torch.from_numpy(np.unpackbits(z[f"mask{i}"], axis=-1, bitorder="little")[..., :mc.keys_of(case, i % 3)].astype(bool))
             for i in range(case.layers)]
    return case, m, torch.from_numpy(z["query_feat"]), masks, z


@pytest.mark.parametrize("fx", [c.name for c in mc.FIXTURES])
def test_restatement_agrees_with_the_reference(fx):
    """The reference's own forward (fp32) against the float64 restatement on the same weights and inputs: every attention-mask bit of
    every layer, as the layer was given it (after the all-masked rule), and the queries after the last layer within 8 x the fp32
    restatement's own error."""
    case, m, q_ref, masks, z = load_fixture(fx)
    assert (case.N, case.Q, case.layers) == next((c.N, c.Q, c.layers) for c in mc.FIXTURES if c.name == fx)
    with torch.no_grad():
        params, (mf, mems) = mc.make_params(case), mc.make_inputs(case)
        rec64, out64 = mc.Restatement(params, mf, mems, torch.float64, case.layers).run()
        _, out32 = mc.Restatement(params, mf, mems, torch.float32, case.layers).run()
    for i in range(case.layers):
        want = rec64[i]["logits"] < 0
        want[want.all(dim=-1)] = False
        assert torch.equal(masks[i], want), i
        chk = z[f"out{i}_checks"]
        assert abs(chk[0] - float(rec64[i]["x_out"].sum())) <= 1e-3 * max(1.0, abs(chk[0]))
    own = float((out32.double() - out64).abs().max())
    err = float((q_ref.double().transpose(0, 1) - out64).abs().max())
    print(f"{fx}: reference vs float64 {err:.3e}, fp32 restatement vs float64 {own:.3e}")
    assert err <= 8 * own
    assert sorted(m["keys"]) == sorted(mc.param_shapes(case.Q, case.K + 1, case.layers))


@pytest.mark.parametrize("name", [c.name for c in mc.CASES])
def test_resize_commutes_with_the_mask_einsum(name):
    """mask_embed . resize(mask_feature) equals resize(mask_embed . mask_feature) in float64 to rounding, at every layer's state: a logit
    is a sum of 256 products of O(1) numbers behind four bilinear taps, so 1e-11 of the largest logit is ~40 ulp of slack."""
    st = mc.study(mc.BY_NAME[name])
    with torch.no_grad():
        for i, l in enumerate(st["layers"]):
            lvl = st["r64"].head_logits_level(l["x_in"], i % 3)
            assert float((lvl - l["logits"]).abs().max()) <= 1e-11 * float(l["logits"].abs().max()), i


def _chunks(S):
    """the key split of axvs_m2f.hip: at least 256 keys per chunk, at most 64 chunks, chunk lengths multiples of 32"""
    n = min(-(-S // 256), 64)
    chunk = -(-(-(-S // n)) // 32) * 32
    return chunk, -(-S // chunk)


@pytest.mark.parametrize("name", [c.name for c in mc.CASES])
def test_case_screening(name):
    """Conditions on the inputs, decided here on the CPU: few logits inside the band (so the bit comparison outside it says something),
    no fp32-vs-float64 bit difference where the end-to-end numbers are compared, and the shapes each case is there for."""
    case = mc.BY_NAME[name]
    st = mc.study(case)
    total = sum(l["logits"].numel() for l in st["layers"])
    for key in ("band_tf", "band_free"):
        inside = sum(int((l["logits"].abs() <= l[key]).sum()) for l in st["layers"])
        assert inside <= 1e-3 * total, (key, inside, total)
    assert {"a", "c", "f"} <= set(mc.NO_FLIP)
    if name in mc.NO_FLIP:
        assert [l["flips32"] for l in st["layers"]] == [0] * case.layers
    if name == "b":
        assert all(mc.keys_of(case, l) % 32 and mc.keys_of(case, l) % 64 for l in range(3))
        assert all(case.hw[0] % s[0] or case.hw[1] % s[1] for s in case.levels)
    if name == "c":
        assert case.Q < 16 and case.T % 2 == 1
    if name == "d":
        assert case.N == 3 and case.T == 1
    if name == "e":
        chunk, n = _chunks(mc.keys_of(case, 2))
        assert n > 1 and mc.keys_of(case, 2) % chunk
    if name == "f":
        assert any(bool(l["masked"].all(-1).any()) for l in st["layers"])
        assert any(bool((~l["masked"]).all(-1).any()) for l in st["layers"])
    assert case.layers == (9 if name in ("a", "b") else 3)


# ---- C-ABI -----------------------------------------------------------------------------------------------------------------------------
def _cfg(**kw):
    from axial_vs_amd import _lib
    d = dict(N=1, Q=100, T=2, C=256, heads=8, ffn=2048, num_layers=9, num_levels=3, K1=41, h=24, w=40, lh=(3, 6, 12), lw=(5, 10, 20),
             return_predictions=0, pos_normalize=1, pos_temperature=10000.0, pos_scale=6.283185307179586)
    d.update(kw)
    d["lh"], d["lw"] = (ctypes.c_int * 3)(*d["lh"]), (ctypes.c_int * 3)(*d["lw"])
    return _lib.AxvsM2fCfg(**d)


def test_size_queries_need_no_gpu():
    from axial_vs_amd import _lib
    L = _lib.lib()
    c = _cfg()
    packed = L.axvs_m2f_decoder_packed_bytes(ctypes.byref(c))
    per_layer = 4 * (2 * 4 * 256 * 256 + 2 * 256 * 2048)          # two attentions (in_proj 3 C^2 + out_proj C^2), the FFN
    assert 9 * per_layer < packed < 1.05 * 9 * per_layer + 4 * (3 * 256 * 256 + 2 * 100 * 256 + 41 * 256) + 65536
    ws = L.axvs_m2f_decoder_workspace_bytes(ctypes.byref(c))
    kv = 4 * 2 * 3 * 256 * 2 * (15 + 60 + 240)                     # keys and values of three layers per level
    assert kv < ws < 4 * kv
    assert 0 < L.axvs_m2f_attn_mask_workspace_bytes(ctypes.byref(c), 2) < ws
    assert 0 < L.axvs_m2f_layer_workspace_bytes(ctypes.byref(c), 8) < ws


@pytest.mark.parametrize("kw,word", [
    (dict(C=128), "256"), (dict(heads=4), "256"), (dict(ffn=1024), "2048"), (dict(num_levels=4), "levels"),
    (dict(num_layers=17), "num_layers"), (dict(num_layers=0), "num_layers"), (dict(Q=257), "Q=257"), (dict(Q=0), "Q=0"),
    (dict(T=17), "T=17"), (dict(N=0), "N=0"), (dict(K1=0), "class"), (dict(h=0), "mask features"),
    (dict(T=16, lh=(3, 6, 1024), lw=(5, 10, 1024)), "level 2"), (dict(lh=(0, 6, 12)), "level 0"),
])
def test_bounds_are_refused_with_a_message(kw, word):
    from axial_vs_amd import _lib
    L = _lib.lib()
    c = _cfg(**kw)
    for fn in (L.axvs_m2f_decoder_packed_bytes, L.axvs_m2f_decoder_workspace_bytes):
        assert fn(ctypes.byref(c)) == 0
        assert word in L.axvs_last_error().decode(), (kw, L.axvs_last_error())
    p = ctypes.c_void_p(0x10000)
    mem = (ctypes.c_void_p * 3)(0x20000, 0x30000, 0x40000)
    assert L.axvs_m2f_decoder_fwd(ctypes.byref(c), p, p, mem, p, None, None, None, None, p, 1 << 40, None) == -1
    assert word in L.axvs_last_error().decode()
    assert L.axvs_m2f_attn_mask_fwd(ctypes.byref(c), p, p, p, 0, p, p, p, 1 << 40, None) == -1
    assert L.axvs_m2f_layer_fwd(ctypes.byref(c), p, 0, p, p, p, p, p, p, 1 << 40, None) == -1


def test_null_pointers_levels_and_short_workspaces_are_refused():
    """made-up non-null pointers: every refusal comes before the device is touched"""
    from axial_vs_amd import _lib
    L = _lib.lib()
    c = _cfg()
    p = ctypes.c_void_p(0x10000)
    mem = (ctypes.c_void_p * 3)(0x20000, 0x30000, 0x40000)
    big = 1 << 40
    assert L.axvs_m2f_decoder_fwd(None, p, p, mem, p, None, None, None, None, p, big, None) == -1
    assert L.axvs_m2f_decoder_fwd(ctypes.byref(c), None, p, mem, p, None, None, None, None, p, big, None) == -1
    assert b"null" in L.axvs_last_error()
    hole = (ctypes.c_void_p * 3)(0x20000, None, 0x40000)
    assert L.axvs_m2f_decoder_fwd(ctypes.byref(c), p, p, hole, p, None, None, None, None, p, big, None) == -1
    assert L.axvs_m2f_decoder_fwd(ctypes.byref(c), p, p, mem, p, None, None, p, None, p, big, None) == -1        # debug bits without flags
    assert b"debug" in L.axvs_last_error()
    want = _cfg(return_predictions=1)
    assert L.axvs_m2f_decoder_fwd(ctypes.byref(want), p, p, mem, p, None, None, None, None, p, big, None) == -1
    assert b"return_predictions" in L.axvs_last_error()
    assert L.axvs_m2f_attn_mask_fwd(ctypes.byref(c), p, p, p, 3, p, p, p, big, None) == -1 and b"level" in L.axvs_last_error()
    assert L.axvs_m2f_layer_fwd(ctypes.byref(c), p, 9, p, p, p, p, p, p, big, None) == -1 and b"layer" in L.axvs_last_error()
    assert L.axvs_m2f_decoder_pack(None, None, ctypes.byref(c), p, None) == -1
    for need, call in (
            (L.axvs_m2f_decoder_workspace_bytes(ctypes.byref(c)),
             lambda n: L.axvs_m2f_decoder_fwd(ctypes.byref(c), p, p, mem, p, None, None, None, None, p, n, None)),
            (L.axvs_m2f_attn_mask_workspace_bytes(ctypes.byref(c), 1), lambda n: L.axvs_m2f_attn_mask_fwd(ctypes.byref(c), p, p, p, 1, p, p, p, n, None)),
            (L.axvs_m2f_layer_workspace_bytes(ctypes.byref(c), 4), lambda n: L.axvs_m2f_layer_fwd(ctypes.byref(c), p, 4, p, p, p, p, p, p, n, None))):
        assert need > 0
        assert call(need - 1) == -2
        err = L.axvs_last_error().decode()
        assert "workspace too small" in err and str(need - 1) in err and str(need) in err
        assert call(-1) == -2


def test_pack_refuses_a_missing_parameter():
    from axial_vs_amd import _lib
    L = _lib.lib()
    c = _cfg(num_layers=2)
    k = ctypes.sizeof(_lib.AxvsM2fLayerParams) // ctypes.sizeof(ctypes.c_void_p)
    layers = (_lib.AxvsM2fLayerParams * 2)(*[_lib.fill(_lib.AxvsM2fLayerParams, [ctypes.c_void_p(0x100000 + 64 * (j * k + i)) for i in range(k)])
                                             for j in range(2)])
    head = _lib.fill(_lib.AxvsM2fHeadParams, [ctypes.c_void_p(0x200000 + 64 * i) for i in range(13)])
    layers[1].ffn2_w = None
    assert L.axvs_m2f_decoder_pack(layers, ctypes.byref(head), ctypes.byref(c), ctypes.c_void_p(0x10000), None) == -1
    assert b"layer 1" in L.axvs_last_error()
