"""CPU: the case table of tests/traj_train_cases.py.  Its cases reach the branches their comments name (the host's tier, LDS, grid and
chunk arithmetic, restated in traj_train_cases.structure), and their inputs are well conditioned: the float64 oracle's own float32 run,
with the same dropout factors, lies within TOL / 10 of it on every measure the GPU test holds the device to, and no hidden unit's ReLU
pre-activation lies within fp32 rounding of zero.  Those are conditions on the inputs, not on the code: a case that misses one gets
another seed, never another bound.  The gradients that are zero in exact arithmetic are the exception, stated where it is made."""
import pytest
import torch

import traj_train_cases as tc


@pytest.mark.parametrize("name", list(tc.CASES))
def test_case_reaches_what_its_comment_claims(name):
    c, s = tc.CASES[name], tc.structure(tc.CASES[name])
    assert set(tc.CLAIMS) == set(tc.CASES)
    assert {k: s[k] for k in tc.CLAIMS[name]} == tc.CLAIMS[name]
    # the bounds of make_dims_any, make_dims and check_frame: these shapes are built, not refused
    assert tc.accepted(c)
    assert c.kind in ("axial", "full") and c.C % 8 == 0


def test_structure_restates_the_host_constants():
    """the figures the host code's comments and the kernels' LDS layouts give"""
    assert tc.spatial_frame_lds(560) == 161280 <= tc.K_MAX_LDS < tc.spatial_frame_lds(561) == 165888
    assert tc.spatial_split_lds(128) == 3 * (128 * 32 + 32 * 132) * 2
    assert tc.spatial_chunk_lds() == 72 * 1024 and tc.spatial_kv_lds(512) == 155648 <= tc.K_MAX_LDS
    assert tc.spatial_grid(512, 5, 3) == (512, 1, 1) and tc.spatial_grid(511, 5, 3) == (511, 1, 3)
    assert tc.spatial_grid(8, 100, 2) == (8, 25, 2) and tc.spatial_grid(2, 36, 1) == (2, 9, 1)
    # the refusals the GPU test asks for lie just outside: T = 17, 321 keys at head_dim 64 on both layers
    assert not tc.accepted(tc.Case("axial", 1, 17, 64, 8, 2, 2, 64, 0, 0, 0, 0))
    assert tc.accepted(tc.Case("full", 1, 1, 128, 2, 16, 20, 64, 0, 0, 0, 0)) and not tc.accepted(tc.Case("full", 1, 1, 128, 2, 3, 107, 64, 0, 0, 0, 0))
    assert tc.accepted(tc.Case("axial", 1, 1, 128, 2, 1, 320, 64, 0, 0, 0, 0)) and not tc.accepted(tc.Case("axial", 1, 1, 128, 2, 1, 321, 64, 0, 0, 0, 0))


def test_table_covers_the_branches_between_its_cases():
    st = {n: tc.structure(c) for n, c in tc.CASES.items()}
    ps = [{k[2:]: v for k, v in s.items() if k.startswith(p + ".")} | dict(case=n, D=s["D"], T=s["T"])
          for n, s in st.items() for p, *_ in tc.passes(tc.CASES[n])]
    assert {p["tier"] for p in ps} == {"Valu", "Split", "Mfma", "Chunk"}
    # both sides of the Split / Mfma and the Mfma / Chunk boundary
    assert {("Split", 128), ("Mfma", 129), ("Mfma", 560), ("Chunk", 561)} <= {(p["tier"], p["L"]) for p in ps}
    assert {1, 2, 3} <= {p["nchunks"] for p in ps} and any(p["nchunks"] > 1 and p["last_chunk_live"] == 1 for p in ps)
    assert any(p["grid_fwd"][1:] == (1, 1) and p["tier"] != "Valu" and p["T"] > 1 for p in ps)           # one workgroup per (sequence, head)
    assert any(p["grid_fwd"][2] > 1 for p in ps) and any(p["grid_fwd"][1] > 1 for p in ps)               # frames and query tiles split
    assert any(p["qtiles_per_wave"] and p["qtiles_per_wave"] > 1 and p["frames_per_wg"] > 1 for p in ps)
    assert {8, 16, 32, 64} == {s["D"] for s in st.values() if s["TMAX"] == 16}
    assert {1, 8, 9, 16} <= {s["T"] for s in st.values()}
    assert any(p["tier"] == "Valu" and p["q_over_64k"] for p in ps) and any(p["tier"] == "Valu" and p["kv_over_64k"] for p in ps)
    assert any(p["tier"] == "Valu" and p["lds_fwd"] == tc.K_MAX_LDS for p in ps)
    assert any(p["tier"] != "Valu" and p["kv_over_64k"] for p in ps) and any(p["tier"] == "Mfma" and p["q_over_64k"] for p in ps)
    assert any(s["colsum"][0] > 64 and s["colsum"][2] < s["colsum"][0] for s in st.values())
    assert any(p["L"] == 1 for p in ps) and any(p["key_chunks"] and p["last_key_chunk"] == 1 for p in ps) and any(p["idle_slots"] for p in ps)
    # T = 1 on the Split and on the VALU kernels; the VALU kernels past 256 for head_dim 16, 32 and 64
    assert {"Split", "Valu"} <= {p["tier"] for p in ps if p["T"] == 1}
    assert {16, 32, 64} <= {p["D"] for p in ps if p["tier"] == "Valu" and p["valu_iters"] > 1}
    # dropout on in at least every second case, and in at least one case of each tier
    on = [n for n, c in tc.CASES.items() if c.p_dropout > 0 and c.p_attn_drop > 0]
    assert 2 * len(on) >= len(tc.CASES)
    assert {p["tier"] for p in ps if p["case"] in on} == {"Valu", "Split", "Mfma", "Chunk"}
    # TWICE: one case with two query chunks, one VALU case past 256
    assert len(tc.TWICE) == 2 and all(n in tc.CASES for n in tc.TWICE)
    assert any(p["case"] in tc.TWICE and p["nchunks"] == 2 for p in ps)
    assert any(p["case"] in tc.TWICE and p["tier"] == "Valu" and p["valu_iters"] > 1 for p in ps)


@pytest.mark.parametrize("name", list(tc.CASES))
def test_float32_oracle_is_within_a_tenth_of_the_tolerance(name):
    c = tc.CASES[name]
    ref64, ref32 = tc.reference(name, torch.float64), tc.reference(name, torch.float32)
    assert tc.all_finite(ref64) and tc.all_finite(ref32)
    # ReLU ties: from float64 alone.  A pre-activation is a sum of C products; fp32 rounds each and their partial sums to 2^-24, so a
    # unit at 2^-21 of sum |z_c w_fc| or more keeps its side in an fp32 forward whatever the summation order
    print(f"{name}: smallest ReLU margin {ref64['relu_margin']:.3e} over {tc.structure(c)['hidden_units']} hidden units")
    assert ref64["relu_margin"] >= tc.RELU_MARGIN
    e = tc.errors(ref32, ref64)
    # Gradients that vanish in exact arithmetic whatever the inputs (traj_train_cases: k.bias; at T = 1 proj_q; at L = 1 q and k.weight).
    # Their measure is rounding noise over the floor, which no seed moves, so TOL / 10 cannot be a condition on the inputs there.  They
    # are recognised from float64 alone, must be exactly the set the structure predicts, and the fp32 noise on them must stay under
    # 1e-7 of the largest gradient norm.
    scale = tc.grad_scale(ref64)
    found = sorted(k for k, v in ref64["grads"].items() if float(v.norm()) < 1e-12 * scale)
    assert found == tc.vanishing(c)
    for k in found:
        noise = float(ref32["grads"][k].double().norm()) / scale
        print(f"{name}: grad.{k} vanishes in exact arithmetic, fp32 noise {noise:.2e} of the largest gradient norm")
        assert noise < tc.VANISH_NOISE
        del e["grad." + k]
    worst = max(e, key=e.get)
    print(f"{name}: fp32 oracle vs float64, worst {worst} {e[worst]:.2e}")
    assert e[worst] < tc.TOL / 10, {k: f"{v:.2e}" for k, v in e.items() if v >= tc.TOL / 10}
