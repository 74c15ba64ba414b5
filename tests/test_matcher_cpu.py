"""CPU: the float64 restatement of the matcher (tests/matcher_cases.py) against the reference's stored fp32 results, and the host side of
the new C-ABI entry points (bindings, refusals before any device work)."""
import ctypes
import re
import os

import pytest
import torch

import __graft_entry__ as ge
import matcher_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def built():
    ge.build()


COMBOS = [(s, kind, mv) for s in mc.SHAPES for kind, mv in mc.combos_of(s)]


@pytest.mark.parametrize("s,kind,mv", COMBOS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_restatement_reproduces_the_reference(s, kind, mv):
    fx = mc.shape_fixture(s)
    assert (kind, mv) in fx.combos
    Q, M, K, T, H, W = s
    ms, cs, C, rows, cols = fx.restated(kind, mv)
    r = fx.ref[(kind, mv)]
    assert torch.equal(rows, r["rows"]) and torch.equal(cols, r["cols"])
    assert len(rows) == min(Q, M) and rows.dtype == torch.int64
    assert torch.equal(C, r["cost64"])                          # the stored float64 cost is this restatement's
    bm, bc = mc.fp32_bound_mask(Q, T * H * W), mc.fp32_bound_class(K + 1)
    e_ms, e_cs = mc.rel_err(r["mask_sim"], ms), mc.rel_err(fx.ref_class_sim, cs)
    e_d, e_c = mc.rel_err(r["dice"], ms[rows, cols]), mc.rel_err(r["cls"], cs[rows, cols])
    print(f"[matcher cpu] {mc.shape_name(s)} {kind} masking={mv}: reference fp32 vs float64 mask_sim {e_ms:.2e} class_sim {e_cs:.2e} "
          f"matched dice {e_d:.2e} cls {e_c:.2e} (bounds {bm:.2e}, {bc:.2e}); yardstick {fx.reference_error(kind, mv):.2e}")
    assert e_ms <= bm and e_d <= bm
    assert e_cs <= bc and e_c <= bc
    assert mc.rel_err(r["cost"], C) <= bm + bc + bm * bc
    assert float(C.abs().max()) <= 0.17                          # the screen's +-1e-6 is stated for costs of this size


@pytest.mark.parametrize("name", mc.E2E)
def test_restatement_reproduces_the_end_to_end_fixtures(name):
    fx = mc.E2EFixture(name)
    m = fx.meta
    assert m["B"] == 2 and m["L"] == 3 and len(set(m["M"])) == 2
    P = m["T"] * m["H"] * m["W"]
    for l, o in enumerate(fx.layers):
        for b, t in enumerate(fx.targets):
            r = fx.ref[l][b]
            assert len(r["rows"]) == min(m["Q"], m["M"][b])
            if m["M"][b] == 0:
                assert r["rows"].numel() == r["cols"].numel() == r["dice"].numel() == r["cls"].numel() == 0
                continue
            ms, cs, C, rows, cols = mc.restate(o["pred_masks"][b], o["pred_logits"][b], t["masks"], t["labels"], m["masking"])
            assert torch.equal(rows, r["rows"]) and torch.equal(cols, r["cols"]) and torch.equal(C, r["cost64"])
            assert mc.stable(C, rows, cols, trials=20)
            assert mc.rel_err(r["dice"], ms[rows, cols]) <= mc.fp32_bound_mask(m["Q"], P)
            assert mc.rel_err(r["cls"], cs[rows, cols]) <= mc.fp32_bound_class(m["K"] + 1)


@pytest.mark.parametrize("s", mc.EDGE_SHAPES, ids=lambda v: "x".join(map(str, v)))
@pytest.mark.parametrize("kind", ["bool", "float"])
@pytest.mark.parametrize("mv", [1, 0])
def test_plain_fp32_evaluation_stays_under_half_the_format_bounds(s, kind, mv):
    """the shapes the GPU test checks without reference fixtures (matcher_cases.EDGE_SHAPES): the restatement's formulas evaluated in
    fp32 by torch on the CPU are within HALF of fp32_bound_mask + fp32_bound_class (mask similarity, cost) and of fp32_bound_class
    (class similarity) of float64, so the bounds leave an honest fp32 kernel room and still sit far below an error of 1 / ntiles or 1 / Q"""
    Q, M, K, T, H, W = s
    P = T * H * W
    pred, logits, labels, targets = mc.edge_inputs(s)
    ms64, cs64, C64, _, _ = mc.restate(pred, logits, targets[kind], labels, mv)
    p = torch.softmax(pred.flatten(1), 0)
    t = targets[kind].float().flatten(1)
    if mv:
        p = p * (t.sum(0, keepdim=True) > 0).float()
    ms = (p @ t.T) / ((p.sum(-1)[:, None] + t.sum(-1)[None, :]) / 2.0 + 1e-5)
    cs = torch.softmax(logits, -1)[:, :-1][:, labels]
    assert ms.dtype == cs.dtype == torch.float32
    bm, bc = mc.fp32_bound_mask(Q, P), mc.fp32_bound_class(K + 1)
    errs = mc.rel_err(ms, ms64), mc.rel_err(cs, cs64), mc.rel_err(-ms * cs, C64)
    print(f"[matcher cpu] edge {s} {kind} masking={mv}: fp32 / bound  mask_sim {errs[0] / (bm + bc):.3f} class_sim {errs[1] / bc:.3f} cost {errs[2] / (bm + bc):.3f}")
    assert errs[0] <= 0.5 * (bm + bc) and errs[2] <= 0.5 * (bm + bc) and errs[1] <= 0.5 * bc
    assert bm + bc < 0.1 / max(Q, (P + 63) // 64)                 # a dropped tile or query changes a value by 1 / ntiles or 1 / Q: over 10 bounds
    assert float(ms64.max()) > 0.0


def _declared_arg_count(name):
    text = open(os.path.join(ROOT, "include", "axvs.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    args = re.search(r"\b" + name + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
    return len([a for a in args.split(",") if a.strip()])


def test_new_symbols_are_bound_with_the_declared_argument_counts():
    from axial_vs_amd import _lib
    L = _lib.lib()
    for name in ("axvs_linear_sum_assignment_rect", "axvs_video_matcher_workspace_bytes", "axvs_video_matcher"):
        assert hasattr(L, name)
        assert len(_lib.SIGNATURES[name][1]) == _declared_arg_count(name), name
    assert _lib.SIGNATURES["axvs_linear_sum_assignment"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p])


def test_wrong_sizes_and_null_pointers_are_refused_before_any_device_work():
    from axial_vs_amd import _lib
    L = _lib.lib()
    rect = L.axvs_linear_sum_assignment_rect
    assert rect(None, 8, 5, 8, None, None, None, 1, None) == -1 and b"null" in L.axvs_last_error()
    assert rect(1, 8, 513, 8, None, 1, 1, 1, None) == -1 and b"512" in L.axvs_last_error()
    assert rect(1, 600, 5, 513, None, 1, 1, 1, None) == -1 and b"512" in L.axvs_last_error()
    assert rect(1, 8, 0, 8, None, 1, 1, 1, None) == -1
    assert rect(1, 8, 5, 8, None, 1, 1, 0, None) == -1
    assert rect(1, 7, 5, 8, None, 1, 1, 1, None) == -1 and b"ld" in L.axvs_last_error()
    assert rect(1, 8, 5, 8, (ctypes.c_int * 2)(3, 9), 1, 1, 2, None) == -1 and b"nc_per_problem" in L.axvs_last_error()
    assert rect(None, 0, 8, 0, None, None, None, 3, None) == 0          # (8, 0): the empty result, nothing to write

    ws = L.axvs_video_matcher_workspace_bytes
    assert ws(4, 1, 128, 96, 65536) > 0 and ws(4, 1, 128, 0, 65536) == 0
    assert ws(8, 1, 128, 96, 65536) >= ws(4, 1, 128, 96, 65536)

    one = (ctypes.c_void_p * 1)(1)
    m1 = (ctypes.c_int * 1)(5)

    def vm(masks=one, mdt=_lib.AXVS_F32, logits=one, tgt=1, tdt=_lib.AXVS_U8, labels=1, m=m1, Ln=1, B=1, Q=16, K1=8, P=120, M_max=5, sims=1, rows=1,
           cols=1, dice=1, cls=1, wsp=1, wsb=1 << 30):
        return L.axvs_video_matcher(masks, mdt, logits, tgt, tdt, labels, m, Ln, B, Q, K1, P, M_max, 1, sims, rows, cols, dice, cls, wsp, wsb, None)

    for kw in (dict(masks=None), dict(logits=None), dict(m=None), dict(tgt=None), dict(labels=None), dict(sims=None), dict(rows=None),
               dict(cols=None), dict(dice=None), dict(cls=None), dict(wsp=None), dict(masks=(ctypes.c_void_p * 1)(None))):
        assert vm(**kw) == -1 and b"null" in L.axvs_last_error(), kw
    for kw in (dict(Ln=0), dict(Ln=17), dict(B=0), dict(B=65), dict(Q=0), dict(Q=513), dict(M_max=513), dict(K1=1), dict(P=0), dict(mdt=7), dict(tdt=0),
               dict(M_max=6), dict(m=(ctypes.c_int * 1)(-1)), dict(Q=512, M_max=96, m=(ctypes.c_int * 1)(96))):
        assert vm(**kw) == -1, kw
    assert vm(wsb=16) == -2 and b"workspace" in L.axvs_last_error()


def test_python_surface_refuses_cpu_tensors():
    import axial_vs_amd as ax
    with pytest.raises(RuntimeError, match="GPU"):
        ax.linear_sum_assignment(torch.zeros(3, 5))
    fx = mc.E2EFixture(mc.E2E[0])
    with pytest.raises(RuntimeError, match="GPU"):
        ax.VideoHungarianMatcher()(fx.outputs(), fx.targets)
    with pytest.raises(RuntimeError, match="GPU"):
        ax.match_layers(fx.outputs(), fx.targets)
    assert ax.VideoHungarianMatcher(masking_void_pixel=False).masking_void_pixel is False
