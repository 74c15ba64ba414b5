"""CPU: the regimes of tests/traj_train_regime_cases.py.  Every stored (case, regime) meets its screening conditions (the float64 logits
are as large or as sharp as the regime says, the keys, key tiles, key chunks and frames that take the weight are where the kernels'
edges lie, the fp32 oracle is finite and within ORACLE_CAP of float64, no ReLU tie); `shift` keeps its promise in float64; and the bounds
the device is held to can tell: each wrong restatement of the softmax in WRONG misses them on a stored pair of the regimes it names.
Conditions on the inputs, not on the code: a pair that misses one gets another seed or gain from the search, never another bound."""
import pytest
import torch

import traj_train_regime_cases as rc
from golden_util import rel_err

PAIRS = rc.pair_ids()


def test_every_pair_of_the_table_is_stored():
    assert set(rc.PAIRS) == set(PAIRS) and len(PAIRS) == 27
    for (name, regime), pair in rc.PAIRS.items():
        assert 0 <= pair.offset < rc.SEEDS
        assert set(pair.mult) == {"shift": {"mk", "mt"}, "sharp_s": {"gs"}, "sharp_t": {"gt"}}[regime]
    # the families and the partial tiles and chunks the table names, from the host arithmetic restated in traj_train_cases.structure
    st = {n: rc.structure(rc.CASES[n]) for n in rc.FAMILY}
    tiers = {n: {st[n][f"{k}.tier"] for k, *_ in rc.passes(rc.CASES[n])} for n in rc.FAMILY}
    assert all(rc.FAMILY[n] in tiers[n] for n in rc.FAMILY)
    assert st["axial_t16_kv_two_chunks"]["w.last_tile_keys"] == 1 and st["axial_t16_kv_two_chunks"]["w.nchunks"] == 2
    assert st["axial_t16_kv_two_chunks"]["TMAX"] == 16 and st["axial_t8"]["TMAX"] == 8 and st["axial_t8"]["T"] == 8
    assert st["full_mfma129"]["t.nkt"] == 9 and st["full_mfma129"]["t.last_tile_keys"] == 1
    assert (st["full_chunk561"]["t.key_chunks"], st["full_chunk561"]["t.last_key_chunk"]) == (3, 49)
    assert (st["full_chunk769"]["t.key_chunks"], st["full_chunk769"]["t.last_key_chunk"]) == (4, 1)
    assert {st[n]["D"] for n in rc.FAMILY if rc.FAMILY[n] == "Valu"} == {8, 16, 64}
    assert (st["axial_d8_t9"]["T"], st["axial_d8_t9"]["TMAX"]) == (9, 16)
    assert st["axial_l1"]["h.L"] == 1 and st["axial_t1"]["T"] == 1
    assert all(st[n]["T"] > 1 for n, r in PAIRS if r == "sharp_t")


@pytest.mark.parametrize("name,regime", PAIRS)
def test_stored_pair_meets_its_screening_conditions(name, regime):
    pair = rc.PAIRS[name, regime]
    misses, report = rc.screen(name, regime, pair.offset, pair.mult)
    print(f"{name} {regime} seed + {pair.offset} {pair.mult}")
    print("\n".join(rc.describe(report)))
    assert not misses, misses
    assert rc.all_finite(rc.reference(name, regime, torch.float32))


@pytest.mark.parametrize("name", list(rc.FAMILY))
def test_shift_leaves_the_float64_step_unchanged(name):
    """q . b_k is a constant per (query, head) over a softmax's logits: out, d_src and d_pos are those of the unshifted weights"""
    assert rc.PAIRS[name, "shift"].mult.get("mq", 1) == 1
    got, want = rc.reference(name, "shift"), rc.plain(name, "shift")
    e = {k: rel_err(got[k], want[k]) for k in ("out", "d_src", "d_pos")}
    print(name, {k: f"{v:.2e}" for k, v in e.items()})
    assert max(e.values()) <= 1e-9, e


def candidates(wrong, regime):
    names = rc.WRONG[wrong][3] or [n for n in sorted(rc.FAMILY, key=lambda n: rc.structure(rc.CASES[n])["hidden_units"])]
    return [n for n in names if (n, regime) in rc.PAIRS]


@pytest.mark.parametrize("wrong,regime", [(w, r) for w, spec in rc.WRONG.items() for r in spec[2]])
def test_the_bounds_tell_a_wrong_softmax(wrong, regime):
    """the fp32 oracle with its softmax stated wrongly, held to the device's bounds: it misses them on a stored pair of the regime
    (the pairs are tried from the smallest case on; the first that tells ends the search)"""
    told = None
    for name in candidates(wrong, regime):
        pair = rc.PAIRS[name, regime]
        c = rc.seeded(name, pair.offset)
        got = rc.run(name, pair.offset, regime, pair.mult, torch.float32, wrong=wrong)
        misses = rc.missed(c, got, rc.reference(name, regime), rc.reference(name, regime, torch.float32))
        print(f"{wrong} on {name} {regime}: {misses[:4] if misses else 'within the bounds'}")
        if misses:
            told = name
            break
    assert told, f"{wrong}: no stored pair of {regime} tells it from the right softmax"
    if wrong == "no_max":
        assert not rc.all_finite(got)


def test_the_right_softmax_restated_passes():
    """the same route with no softmax swapped is within the bounds: `missed` does not fail everything"""
    name, regime = "axial_t8", "sharp_s"
    pair = rc.PAIRS[name, regime]
    ref32 = rc.reference(name, regime, torch.float32)
    assert not rc.missed(rc.seeded(name, pair.offset), ref32, rc.reference(name, regime), ref32)
