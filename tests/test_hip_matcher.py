"""GPU: rectangular linear sum assignment and the fused VideoHungarianMatcher against SciPy, the float64 restatement and the reference's
stored results (tests/matcher_cases.py, fixtures tests/golden/g18_matcher_*).

The per-element test prints, per fixture, how far the device's mask similarity / class similarity / cost are from float64 in units of
the reference's own fp32 error; the bound is 8 (measured on an MI355X: 0.16 .. 1.20, profiles/matcher_parity.txt)."""
import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment as scipy_lsa

import __graft_entry__ as ge
import matcher_cases as mc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def built():
    ge.build()
    assert torch.cuda.is_available()


LSAP_SHAPES = [(1, 1), (1, 7), (7, 1), (5, 16), (16, 5), (63, 64), (64, 65), (65, 128), (128, 23), (100, 300), (300, 100), (512, 17), (8, 0)]


def _scipy_pairs(c):
    r, k = scipy_lsa(c.astype(np.float64))
    return r.astype(np.int64), k.astype(np.int64)


@pytest.mark.parametrize("n,m", LSAP_SHAPES, ids=lambda v: str(v))
def test_rectangular_assignment_equals_scipy_bit_for_bit(n, m):
    """batches of 3 on the same fp32 matrices: uniform floats; small integers {0..3} (many optima tie) with one constant matrix; and a
    ragged batch whose problems use m, about m / 2 and 1 of the stored columns"""
    import axial_vs_amd as ax
    rng = np.random.default_rng(1000 * n + m)
    uniform = rng.random((3, n, m), dtype=np.float32)
    ties = rng.integers(0, 4, (3, n, m)).astype(np.float32)
    ties[2] = 2.5
    square = [m] * 3 if n == m else None          # a square input keeps the square form (column indices alone) unless num_cols is given
    for kind, cost in (("uniform", uniform), ("ties", ties)):
        rows, cols = ax.linear_sum_assignment(torch.from_numpy(cost).cuda(), num_cols=square)
        assert rows.dtype == cols.dtype == torch.int64 and rows.is_cuda and rows.shape == cols.shape == (3, min(n, m))
        rows, cols = rows.cpu().numpy(), cols.cpu().numpy()
        for z in range(3):
            r, k = _scipy_pairs(cost[z])
            assert np.array_equal(rows[z], r) and np.array_equal(cols[z], k), (kind, z)
    if n != m:
        r1, k1 = ax.linear_sum_assignment(torch.from_numpy(uniform[1]).cuda())       # [n, m] input: unbatched pair
        r, k = _scipy_pairs(uniform[1])
        assert np.array_equal(r1.cpu().numpy(), r) and np.array_equal(k1.cpu().numpy(), k)
    if m >= 2:
        ncs = [m, (m + 1) // 2, 1]
        for kind, cost in (("uniform", uniform), ("ties", ties)):
            rows, cols = ax.linear_sum_assignment(torch.from_numpy(cost).cuda(), num_cols=ncs)
            rows, cols = rows.cpu().numpy(), cols.cpu().numpy()
            for z, nc in enumerate(ncs):
                r, k = _scipy_pairs(cost[z][:, :nc])
                kk = len(r)
                assert np.array_equal(rows[z, :kk], r) and np.array_equal(cols[z, :kk], k), (kind, z, nc)
                assert (rows[z, kk:] == -1).all() and (cols[z, kk:] == -1).all()


def test_square_problems_keep_their_result_and_form():
    import axial_vs_amd as ax
    rng = np.random.default_rng(5)
    cost = rng.random((3, 65, 65), dtype=np.float32)
    out = ax.linear_sum_assignment(torch.from_numpy(cost).cuda())
    assert isinstance(out, torch.Tensor) and out.shape == (3, 65)
    rows, cols = ax.linear_sum_assignment(torch.from_numpy(cost).cuda(), num_cols=[65, 65, 65])      # the rectangular kernel on square problems
    for z in range(3):
        r, k = _scipy_pairs(cost[z])
        assert np.array_equal(out[z].cpu().numpy(), k) and np.array_equal(cols[z].cpu().numpy(), k) and np.array_equal(rows[z].cpu().numpy(), r)
    with pytest.raises(RuntimeError, match="512"):
        ax.linear_sum_assignment(torch.zeros(513, 4, device="cuda"))


def _gpu_inputs(fx, kind, dtype=torch.float32):
    out = {"pred_masks": fx.pred.cuda().to(dtype)[None], "pred_logits": fx.logits.cuda()[None]}
    tg = [{"labels": fx.labels.cuda(), "masks": fx.targets[kind].cuda()}]
    return out, tg


PARITY_CASES = [(s, kind, mv, torch.float32) for s in mc.SHAPES for kind, mv in mc.combos_of(s)] + \
               [(mc.SHAPES[0], "bool", 1, torch.float16), (mc.SHAPES[1], "float", 0, torch.float16), (mc.SHAPES[3], "bool", 1, torch.bfloat16)]


@pytest.mark.parametrize("s,kind,mv,dtype", PARITY_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v).replace("torch.", ""))
def test_similarity_and_cost_per_element_against_float64(s, kind, mv, dtype):
    """every element of mask similarity, class similarity and cost within 8x the reference's own fp32 error on the fixture (relative,
    against float64); the assignment on the device's cost equals the reference's (the fixtures are screened for stability)"""
    import axial_vs_amd as ax
    fx = mc.shape_fixture(s)
    Q, M = s[0], s[1]
    out, tg = _gpu_inputs(fx, kind, dtype)
    if dtype == torch.bfloat16:
        # the stored logits are fp16 values: rounded to bf16 they are other numbers, so the float64 restatement is taken on the rounded
        # values; the yardstick stays the reference's fp32 error on this shape and flag combination
        ms64, cs64, C64, rows64, cols64 = mc.restate(fx.pred.bfloat16().float(), fx.logits, fx.targets[kind], fx.labels, mv)
    else:
        ms64, cs64, C64, rows64, cols64 = fx.restated(kind, mv)
    yard = fx.reference_error(kind, mv)
    (ms, cs, C), = ax.matcher_costs(out, tg, masking_void_pixel=bool(mv))
    assert ms.shape == cs.shape == C.shape == (Q, M) and C.dtype == torch.float32
    errs = [mc.rel_err(ms, ms64), mc.rel_err(cs, cs64), mc.rel_err(C, C64)]
    print(f"[matcher parity] {mc.shape_name(s)} {kind} masking={mv} {str(dtype).replace('torch.', '')}: reference fp32 error {yard:.2e}; device / reference: "
          f"mask_sim {errs[0] / yard:.2f} class_sim {errs[1] / yard:.2f} cost {errs[2] / yard:.2f}")
    assert 5e-8 < yard < 2e-6                                   # an fp32 computation's error: the yardstick itself is sane
    assert max(errs) <= 8.0 * yard, errs
    ind, dice, cls = ax.VideoHungarianMatcher(masking_void_pixel=bool(mv))(out, tg)
    r = fx.ref[(kind, mv)]
    if dtype != torch.bfloat16:
        assert torch.equal(ind[0][0].cpu(), r["rows"]) and torch.equal(ind[0][1].cpu(), r["cols"])
    else:
        # the stored indices belong to the unrounded logits: compare with the float64 optimum on the rounded ones, screened like a fixture
        assert mc.stable(C64, rows64, cols64)
        assert torch.equal(ind[0][0].cpu(), rows64) and torch.equal(ind[0][1].cpu(), cols64)
    assert torch.equal(dice[0], ms[ind[0][0], ind[0][1]]) and torch.equal(cls[0], cs[ind[0][0], ind[0][1]])      # device indices index device tensors


@pytest.mark.parametrize("s", mc.EDGE_SHAPES, ids=lambda v: "x".join(map(str, v)))
@pytest.mark.parametrize("kind", ["bool", "float"])
@pytest.mark.parametrize("mv", [1, 0])
def test_similarity_at_ragged_query_counts_and_pixel_splits_against_float64(s, kind, mv):
    """the shapes the fixtures' grid leaves out (matcher_cases.EDGE_SHAPES: Q = 5 and 3, a ragged split of 5 tiles, one partial tile,
    two block chunks on two pixel workgroups), without reference fixtures: every element against the float64 restatement at the
    format-derived bounds, fp32_bound_mask + fp32_bound_class for mask similarity and cost, fp32_bound_class for class similarity.
    A plain fp32 evaluation stays under half of them (tests/test_matcher_cpu.py); they are there to catch a dropped tile, a skipped
    partial or a wrong chunk (errors of 1 / ntiles or 1 / Q), not to measure rounding.  The assignment is SciPy's on the device's cost."""
    import axial_vs_amd as ax
    from axial_vs_amd import _lib
    Q, M, K, T, H, W = s
    P = T * H * W
    pred, logits, labels, targets = mc.edge_inputs(s)
    ms64, cs64, C64, _, _ = mc.restate(pred, logits, targets[kind], labels, mv)
    out = {"pred_masks": pred.cuda()[None], "pred_logits": logits.cuda()[None]}
    tg = [{"labels": labels.cuda(), "masks": targets[kind].cuda()}]
    if P > 256:           # split over pixel workgroups (a workgroup's partial sums are Q M + Q + M floats); with Q = 260 on two block chunks
        assert _lib.lib().axvs_video_matcher_workspace_bytes(1, 1, Q, M, P) >= 2 * (Q * M + Q + M) * 4
    (ms, cs, C), = ax.matcher_costs(out, tg, masking_void_pixel=bool(mv))
    assert ms.shape == cs.shape == C.shape == (Q, M)
    bm, bc = mc.fp32_bound_mask(Q, P), mc.fp32_bound_class(K + 1)
    errs = [mc.rel_err(ms, ms64), mc.rel_err(cs, cs64), mc.rel_err(C, C64)]
    print(f"[matcher edge] Q{Q} M{M} P{P} {kind} masking={mv}: error / bound  mask_sim {errs[0] / (bm + bc):.4f} class_sim {errs[1] / bc:.4f} "
          f"cost {errs[2] / (bm + bc):.4f}")
    assert errs[0] <= bm + bc and errs[2] <= bm + bc and errs[1] <= bc, errs
    ind, dice, cls = ax.VideoHungarianMatcher(masking_void_pixel=bool(mv))(out, tg)
    r, k = _scipy_pairs(C.cpu().numpy())
    assert np.array_equal(ind[0][0].cpu().numpy(), r) and np.array_equal(ind[0][1].cpu().numpy(), k)
    assert torch.equal(dice[0], ms[ind[0][0], ind[0][1]]) and torch.equal(cls[0], cs[ind[0][0], ind[0][1]])


def _e2e_restated(fx):
    """float64 matched values of every (layer, video) with objects, and the reference's own fp32 error on them pooled over the fixture:
    the yardstick of the end-to-end matched values (8x, like the per-element test)"""
    m, out, yard = fx.meta, {}, 0.0
    for l, o in enumerate(fx.layers):
        for b, t in enumerate(fx.targets):
            if m["M"][b] == 0:
                continue
            ms, cs, _, rows, cols = mc.restate(o["pred_masks"][b], o["pred_logits"][b], t["masks"], t["labels"], m["masking"])
            out[(l, b)] = (ms[rows, cols], cs[rows, cols])
            yard = max(yard, mc.rel_err(fx.ref[l][b]["dice"], ms[rows, cols]), mc.rel_err(fx.ref[l][b]["cls"], cs[rows, cols]))
    return out, yard


def _check_layer(got, l, fx, restated, yard):
    ind, dice, cls = got
    m = fx.meta
    assert len(ind) == len(dice) == len(cls) == m["B"]
    for b in range(m["B"]):
        r = fx.ref[l][b]
        k = min(m["Q"], m["M"][b])
        assert isinstance(ind[b], tuple) and ind[b][0].dtype == ind[b][1].dtype == torch.int64 and ind[b][0].is_cuda
        assert ind[b][0].shape == ind[b][1].shape == dice[b].shape == cls[b].shape == (k,) and dice[b].dtype == cls[b].dtype == torch.float32
        assert torch.equal(ind[b][0].cpu(), r["rows"]) and torch.equal(ind[b][1].cpu(), r["cols"])
        if k == 0:
            continue
        d64, c64 = restated[(l, b)]
        errs = (mc.rel_err(dice[b], d64), mc.rel_err(cls[b], c64))
        assert max(errs) <= 8.0 * yard, (l, b, errs, yard)


@pytest.mark.parametrize("name", mc.E2E)
def test_end_to_end_matches_the_reference_and_repeats_bit_for_bit(name):
    """B = 2 videos with different object counts (one fixture has a video without objects), 3 layers: VideoHungarianMatcher.forward on the
    final prediction and match_layers on all of them give the reference's indices and matched values; a second run is bit-equal"""
    import axial_vs_amd as ax
    fx = mc.E2EFixture(name)
    L = fx.meta["L"]
    out, tg = fx.outputs("cuda"), fx.targets_on("cuda")
    matcher = ax.VideoHungarianMatcher(masking_void_pixel=bool(fx.meta["masking"]))
    restated, yard = _e2e_restated(fx)
    assert 5e-8 < yard < 2e-6
    single = matcher(out, tg)
    _check_layer(single, L - 1, fx, restated, yard)
    layers = ax.match_layers(out, tg, masking_void_pixel=bool(fx.meta["masking"]))
    assert len(layers) == L
    order = [L - 1] + list(range(L - 1))                       # entry 0: the final prediction, entry 1 + i: aux_outputs[i]
    for got, l in zip(layers, order):
        _check_layer(got, l, fx, restated, yard)
    again = ax.match_layers(out, tg, masking_void_pixel=bool(fx.meta["masking"]))
    for a, b in zip(layers + [single], again + [layers[0]]):
        for v in range(fx.meta["B"]):
            assert torch.equal(a[0][v][0], b[0][v][0]) and torch.equal(a[0][v][1], b[0][v][1])
            assert torch.equal(a[1][v], b[1][v]) and torch.equal(a[2][v], b[2][v])


def test_no_host_synchronisation():
    import axial_vs_amd as ax
    fx = mc.E2EFixture(mc.E2E[1])
    out, tg = fx.outputs("cuda"), fx.targets_on("cuda")
    cost = torch.rand(3, 20, 33, device="cuda")
    matcher = ax.VideoHungarianMatcher()
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        layers = ax.match_layers(out, tg)
        single = matcher(out, tg)
        pair = ax.linear_sum_assignment(cost, num_cols=[33, 20, 5])
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert torch.equal(layers[0][0][0][0], single[0][0][0]) and pair[0].shape == (3, 20)
