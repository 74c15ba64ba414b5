"""CPU: the cases of tests/attention_edge_cases.py are what they claim to be and can tell a wrong attention from the right one.

The hand-built masks have the rows they are named after; the solved mask features give the float64 mask head rows with one open key, none
and all, with no logit near the rounding band; at the sharpest class the float64 softmax of each kernel is almost one-hot, past fp32 exp's
overflow without the max subtraction and past its underflow, at class 0 it is uniform; and each wrong restatement (no max subtraction, a
chunk-local maximum, uniform weights for a masked chunk, no all-masked rule) misses the bound the device is held to.  The factors by which
they miss are printed, and appended to the file AXVS_WRITE_PARITY names (profiles/attention_edges_parity.txt)."""
import math
import os
import re

import pytest
import torch

import attention_edge_cases as ec
import m2f_decoder_cases as mc

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "axial_vs_amd", "csrc")


def note(line):
    print(line)
    if os.environ.get("AXVS_WRITE_PARITY"):
        with open(os.environ["AXVS_WRITE_PARITY"], "a") as f:
            f.write(line + "\n")


def miss(got, item):
    """by what factor `got` misses the bound of `item` (inf: not finite); above 1 the device test would fail"""
    if not bool(torch.isfinite(got).all()):
        return math.inf
    return ec.err(got, item["want"]) / item["tol"]


# ---- A: the split and the masks ---------------------------------------------------------------------------------------------------------------
def test_key_split_is_the_librarys():
    """the restated chunk_of() gives the split the cases are built for (598 keys: three chunks of 224; 16928 keys: 59 of 288), and the
    library's source still states the same split, so that a change of it is noticed here"""
    assert [ec.chunk_of(S) for S in (24, 70, 598)] == [32, 96, 224] and [ec.chunks_of(S) for S in (24, 70, 598)] == [1, 1, 3]
    assert 598 - 2 * 224 == 150                                              # the last of the three chunks is partial
    S = mc.keys_of(ec.CAP, 0)
    assert S == 16928 > ec.MAX_CHUNKS * ec.KEY_CHUNK and ec.chunks_of(S) == 64 and ec.chunk_of(S) == 288 and math.ceil(S / 288) == 59
    with open(os.path.join(CSRC, "axvs_m2f.h")) as f:
        h = f.read()
    with open(os.path.join(CSRC, "axvs_m2f.hip")) as f:
        hip = re.sub(r"\s+", " ", f.read())
    assert re.search(r"kM2fKeyChunk = (\d+);", h).group(1) == str(ec.KEY_CHUNK) and re.search(r"kM2fMaxChunks = (\d+);", h).group(1) == str(ec.MAX_CHUNKS)
    assert "int chunks_of(int S) { return std::min((S + kM2fKeyChunk - 1) / kM2fKeyChunk, kM2fMaxChunks); }" in hip
    assert "int chunk_of(int S) { return ((S + chunks_of(S) - 1) / chunks_of(S) + 31) / 32 * 32; }" in hip
    assert "a.chunk = chunk_of(S), a.nchunk = (S + a.chunk - 1) / a.chunk;" in hip


@pytest.mark.parametrize("S", [24, 70, 598])
def test_hand_masks_are_what_they_are_named(S):
    Q, chunk = 100, ec.chunk_of(S)
    n = math.ceil(S / chunk)
    masks = ec.hand_masks(S, chunk, Q)
    is_open = {k: ~m[0] for k, m in masks.items()}
    k = torch.arange(S)
    # one_open: one open key per row, at each listed position that exists, in every full query tile
    want = [p for p in (0, 15, 16, 31, 32, chunk - 1, chunk, 2 * chunk - 1, S - 2, S - 1) if 0 <= p < S]
    assert ec.one_open_positions(S, chunk) == list(dict.fromkeys(want)) and S - 1 in want and 0 in want
    o = is_open["one_open"]
    assert bool((o.sum(-1) == 1).all())
    for tile in range(Q // 16):
        assert sorted(set(o[16 * tile:16 * tile + 16].float().argmax(-1).tolist())) == sorted(set(want)), tile
    # one_chunk: the open keys of a row lie in one chunk; each chunk is the live one in some row of every full tile; one row has only S - 1
    o = is_open["one_chunk"]
    live = torch.stack([o[:, c * chunk:(c + 1) * chunk].any(-1) for c in range(n)], 1)          # [Q, n]
    assert bool((live.sum(-1) == 1).all())
    for tile in range(Q // 16):
        assert bool(live[16 * tile:16 * tile + 16].any(0).all()), tile
    full = o.sum(-1) > 1
    assert bool((o[full].sum(-1) == torch.tensor([min(chunk, S - c * chunk) for c in live[full].float().argmax(-1).tolist()])).all())
    assert bool(((o.sum(-1) == 1) & o[:, S - 1]).any())
    # head_step_masked: every chunk is live and its first 16 keys are masked
    o = is_open["head_step_masked"]
    for c in range(n):
        assert not bool(o[:, c * chunk:c * chunk + 16].any()) and bool(o[:, c * chunk + 16:(c + 1) * chunk].any(-1).all()), c
    # tail_word: open keys in the last 32-bit word only, all of it
    o = is_open["tail_word"]
    lo = 32 * (S // 32) if S % 32 else S - 32
    assert bool(o[:, lo:].all()) and not bool(o[:, :lo].any()) and (S % 32 == 0 or S - lo == S % 32)
    # alternate: keys of one parity, or 16-key steps of one parity
    o = is_open["alternate"]
    assert torch.equal(o[0], k % 2 == 0) and torch.equal(o[1], k % 2 == 1) and torch.equal(o[2], (k // 16) % 2 == 0) and torch.equal(o[3], (k // 16) % 2 == 1)
    assert bool(is_open["all_open"].all()) and not bool(is_open["all_masked"].any())
    if S == 598:       # the three-chunk level has what the split-key combine can get wrong
        assert n == 3 and bool((live.sum(0) > 0).all())
        assert bool((~is_open["one_open"][:, :chunk].any(-1)).any())           # a wholly masked chunk in front of the live one


def test_masks_at_the_chunk_cap():
    c = ec.cap_inputs()
    S, chunk, n = c["S"], c["chunk"], c["nchunk"]
    assert (S, chunk, n) == (16928, 288, 59) and S - (n - 1) * chunk == 224       # the last chunk is partial
    o = ~c["masks"]["one_open"][0]
    assert bool((o.sum(-1) == 1).all()) and o.float().argmax(-1).tolist() == [0, 32, 287, 288, 30 * 288 + 17, 58 * 288 - 1, S - 2, S - 1]
    o = ~c["masks"]["one_chunk"][0]
    live = [sorted(set((torch.nonzero(r).flatten() // chunk).tolist())) for r in o]
    assert live == [[0], [30], [58], [58]] * 2 and int(o[3].sum()) == 1 and bool(o[3, S - 1]) and int(o[2].sum()) == 224
    frac = float((~c["masks"]["half"]).float().mean())
    assert 0.49 < frac < 0.51


def test_written_out_attention_is_the_modules():
    """M2fEdge (nn.MultiheadAttention written out, what the wrong forms and the recorded scores rest on) equals mc.Restatement in float64"""
    for name in ec.M2F_SHARP_CASES:
        for g, a in ec.m2f_variants():
            for i, l in enumerate(ec.m2f_sharp_study(name, g, a)["layers"]):
                assert ec.err(l["written_out"], l["want"]) < 1e-12, (name, g, a, i)
    st = ec.m2f_mask_study(2)
    base = st["st"]
    r = ec.M2fEdge(base["params"], base["mf"], base["mems"], torch.float64, base["case"].layers)
    with torch.no_grad():
        for k, it in st["items"].items():
            assert ec.err(r.layer(2, st["x_in"], it["masked"]), it["want"]) < 1e-12, k


# ---- B: the mask head's rows --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [0, 1, 2])
def test_sparse_rows_exist_and_the_band_is_empty(level):
    st = ec.sparse_rows_study(level)
    S, logits = st["S"], st["logits"]
    assert float(logits.abs().min()) > 1000 * st["band"]                         # no |logit| inside the 8 x band: every bit and flag is compared
    is_open = logits[0] >= 0
    assert torch.equal(is_open, st["is_open"][0])
    n_open = is_open.sum(-1)
    one = n_open == 1
    where = set(is_open[one].float().argmax(-1).tolist())
    tail = 32 * (S // 32) if S % 32 else S - 32
    assert {0, S - 1, tail} <= where, where                                      # key 0, the last key, one in the (partial) last word
    assert bool((n_open == 0).any()) and bool((n_open == S).any())
    print(f"level {level}: S {S}, band {st['band']:.2e}, min |logit| {float(logits.abs().min()):.6f}, one-open rows at keys {sorted(where)}, "
          f"{int((n_open == 0).sum())} all-masked and {int((n_open == S).sum())} all-open rows")


# ---- C: the conditions on the float64 run -----------------------------------------------------------------------------------------------------------
def _sharp_stats():
    """(kernel, tag, row_stats) of every softmax of the sharpest class"""
    out = []
    for name in ec.M2F_SHARP_CASES:
        for a in (0, 1):
            for i, l in enumerate(ec.m2f_sharp_study(name, ec.SHARP["m2f"], a)["layers"]):
                out.append(("m2f", f"case {name} attention {a} layer {i}", l["stats"]))
    for name in ec.KMAX_SHARP_CASES:
        out.append(("kmax", f"case {name}", ec.kmax_sharp_study(name, f"g{ec.SHARP['kmax']}")["stats"]))
    for spec in ec.KPIX_SHARP_CASES:
        for axis in (0, 1):
            out.append(("kpix", f"{spec} axis {axis}", ec.kpix_sharp_study(spec, ec.SHARP["kpix"], axis)["stats"]))
    return out


def test_sharp_conditions():
    """At the sharpest class, every softmax of every case: the median row is almost one-hot, a score is past fp32 exp's overflow, a row's
    score range past its underflow.  (SHARP is the first of 64, 128, ... that gives this.)"""
    for kernel, tag, s in _sharp_stats():
        top, smax, srange = float(s["top"].median()), float(s["smax"].max()), float(s["srange"].max())
        print(f"{kernel} g {ec.SHARP[kernel]} {tag}: median largest weight {top:.4f}, largest score {smax:.1f}, largest range {srange:.1f}")
        assert top > 0.9 and smax > ec.EXP_OVERFLOW and srange > ec.EXP_UNDERFLOW, (kernel, tag)


def test_sharp_is_the_first_factor_that_suffices():
    assert all(g >= 64 and g & (g - 1) == 0 for g in ec.SHARP.values())
    assert ec.SHARP == dict(m2f=64, kmax=64, kpix=64)          # 64 meets the conditions for all three: nothing had to be doubled


def test_class_0_is_uniform():
    """every row's weights are 1 / (its open keys) to 1e-12"""
    for name in ec.M2F_SHARP_CASES:
        for a in (0, 1):
            for l in ec.m2f_sharp_study(name, 0, a)["layers"]:
                assert float(l["stats"]["uniform"].max()) < 1e-12 and float(l["stats"]["srange"].max()) == 0.0, (name, a)
    for name in ec.KMAX_SHARP_CASES:
        assert float(ec.kmax_sharp_study(name, "g0")["stats"]["uniform"].max()) < 1e-12, name
    for spec in ec.KPIX_SHARP_CASES:
        for axis in (0, 1):
            assert float(ec.kpix_sharp_study(spec, 0, axis)["stats"]["uniform"].max()) < 1e-12, (spec, axis)


def test_the_bias_class_moves_the_scores_and_not_the_weights():
    for name in ec.KMAX_SHARP_CASES:
        a, b = ec.kmax_sharp_study(name, "g1"), ec.kmax_sharp_study(name, "bias50")
        assert abs(float((b["stats"]["smax"] - a["stats"]["smax"]).mean()) - 50.0) < 1.0      # the norm adds its bias behind the gain
        assert ec.err(a["want"], b["want"]) < 1e-10, name


def test_floor_of_the_bound():
    want = torch.tensor([1.0, -4.0], dtype=torch.float64)
    assert ec.bound(want.float(), want) == (8 * 4.0 * 2.0 ** -24, 0.0, True)
    tol, own, floor = ec.bound((want + 1e-5).float(), want)
    assert not floor and abs(own - 1e-5) < 1e-6 and tol == 8 * own


# ---- D: the cases can tell ----------------------------------------------------------------------------------------------------------------------------
def test_cases_tell_a_softmax_without_the_max_subtraction():
    """float32, exp(s) / sum exp(s): at the sharpest class it misses in every case of every kernel; at class 1, where the kernels' own
    case files draw from, it passes everywhere (what this set of cases is for)"""
    for g_of, must in ((lambda k: 1, False), (lambda k: ec.SHARP[k], True)):
        rows = []
        for name in ec.M2F_SHARP_CASES:
            g = g_of("m2f")
            for a in (0, 1) if g != 1 else (0,):
                right, bad = ec.m2f_sharp_study(name, g, a), ec.m2f_sharp_study(name, g, a, "no_max")
                rows.append((f"m2f g {g} case {name} attention {a}", max(miss(b, l) for b, l in zip(bad, right["layers"]))))
        for name in ec.KMAX_SHARP_CASES:
            g = g_of("kmax")
            rows.append((f"kmax g {g} case {name}", miss(ec.kmax_sharp_study(name, f"g{g}", "no_max"), ec.kmax_sharp_study(name, f"g{g}"))))
        for spec in ec.KPIX_SHARP_CASES:
            for axis in (0, 1):
                g = g_of("kpix")
                rows.append((f"kpix g {g} {spec} axis {axis}", miss(ec.kpix_sharp_study(spec, g, axis, "no_max"), ec.kpix_sharp_study(spec, g, axis))))
        for tag, f in rows:
            note(f"wrong no_max, {tag}: {f:.3g} x the bound")
            assert (f > 1) == must, tag


def _wrong_on_masks(wrong):
    """mask name -> factor, for layer 2 of case e (three key chunks) and for the cap case"""
    out = {}
    with torch.no_grad():
        st = ec.m2f_mask_study(2)
        base = st["st"]
        r = ec.M2fEdge(base["params"], base["mf"], base["mems"], torch.float64, base["case"].layers, wrong)
        for k, it in st["items"].items():
            out["e layer 2 " + k] = miss(r.layer(2, st["x_in"], it["masked"]), it)
        cap = ec.m2f_cap_study()
        r = ec.M2fEdge(cap["params"], cap["mf"], cap["mems"], torch.float64, 1, wrong)
        for k, it in cap["items"].items():
            out["cap " + k] = miss(r.layer(0, cap["x_in"], it["masked"]), it)
    for k, f in out.items():
        note(f"wrong {wrong}, {k}: {f:.3g} x the bound")
    return out


def test_cases_tell_a_chunk_local_maximum():
    f = _wrong_on_masks("chunk_local_max")
    assert f["e layer 2 one_chunk"] > 1 and f["e layer 2 one_open"] > 1          # a wholly masked chunk: exp(-inf - -inf)
    assert f["e layer 2 alternate"] > 1 and f["e layer 2 head_step_masked"] > 1 and math.isfinite(f["e layer 2 alternate"])      # every chunk live: the missing rescale alone
    assert f["cap one_chunk"] > 1 and f["cap one_open"] > 1 and f["cap half"] > 1 and math.isfinite(f["cap half"])


def test_cases_tell_uniform_weights_for_a_masked_chunk():
    f = _wrong_on_masks("masked_chunk_uniform")
    for k in ("e layer 2 one_open", "e layer 2 one_chunk", "cap one_open", "cap one_chunk"):
        assert f[k] > 1 and math.isfinite(f[k]), k
    for k in ("e layer 2 alternate", "e layer 2 head_step_masked", "e layer 2 all_open", "cap half"):      # no chunk is wholly masked there
        assert f[k] < 1e-6, k


def test_cases_tell_a_missing_all_masked_rule():
    f = _wrong_on_masks("no_all_masked_rule")
    assert f["e layer 2 all_masked"] > 1 and math.isfinite(f["e layer 2 all_masked"])
    assert all(v < 1e-6 for k, v in f.items() if k != "e layer 2 all_masked")
