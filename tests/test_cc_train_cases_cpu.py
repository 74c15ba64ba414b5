"""CPU: the case table of tests/cc_train_cases.py.  Its cases reach the branches their comments name (the host's plan arithmetic,
restated in cc_train_cases.structure), and their inputs are well conditioned: the float64 oracle's own float32 run, with the same
dropout factors, lies within TOL / 10 of it on every measure the GPU test holds the device to -- every output, d_clip_query, every
parameter gradient, every BatchNorm site's batch mean and unbiased variance of every layer.  That is a condition on the inputs, not on
the code: a case that misses it gets another seed or scale, never another bound.  The gradients that are zero in exact arithmetic are
the exception, stated where it is made."""
import pytest
import torch

import cc_train_cases as cc


@pytest.mark.parametrize("name", list(cc.CASES))
def test_case_reaches_what_its_comment_claims(name):
    c, s = cc.CASES[name], cc.structure(cc.CASES[name])
    assert set(cc.CLAIMS) == set(cc.CASES)
    assert {k: s[k] for k in cc.CLAIMS[name]} == cc.CLAIMS[name]
    # the bounds of make_cc_shape: these shapes are built, not refused
    assert c.Q % 8 == 0 and 1 <= c.Tc <= 16 and c.B * c.Tc <= 1024 and s["E"] % 4 == 0 and all(r > 0 for r in c.rates)


def test_table_covers_the_branches_between_its_cases():
    st = {n: cc.structure(c) for n, c in cc.CASES.items()}
    assert any(s["fused"] and s["p_mod"] for s in st.values()) and any(s["fused"] and s["qtiles"] == 2 for s in st.values())
    assert any(not s["fused"] and s["scalar_blocks"] > 1 and s["scalar_last_block"] < s["scalar_per_block"] for s in st.values())
    assert any(s["B"] > 1 and s["z"] > 1 for s in st.values()) and any(s["B"] == 1 and s["z"] > 1 for s in st.values())
    assert {1, 16} <= {c.Tc for c in cc.CASES.values()} and any(s["P"] % 2 for s in st.values()) and any(s["K1"] == 2 for s in st.values())
    assert max(s["entries"] for s in st.values() if s["B"] > 2) > 12
    assert any(c.p_attn_drop > 0 and c.p_aspp_drop > 0 for c in cc.CASES.values())
    assert all(n in cc.CASES for n in cc.TWICE)


def test_running_means_are_of_order_one():
    for c in cc.CASES.values():
        w = cc.make_weights(c)
        for s in cc.BN_SITES:
            m = w[s + ".running_mean"].abs()
            assert 0.25 <= float(m.min()) and float(m.max()) <= 1.5, s


def test_statistics_solve_amplifies_buffer_rounding_by_at_most_16():
    """layer_stats recovers each layer's batch statistics from L buffers; the inverse of its system has absolute row sums of at most 1, 3
    and 16 for L = 1, 2, 3, so one fp32 rounding of a buffer (2^-24) is at most 1e-6 in a statistic, a hundredth of TOL."""
    assert max(c.layers for c in cc.CASES.values()) <= len(cc.STAT_MOMENTA) == 3
    assert [round(cc.stat_solve_amplification(L), 9) for L in (1, 2, 3)] == [1.0, 3.0, 16.0]
    assert 16 * cc.FLOOR < cc.TOL / 100
    # and the solve gives back what went in: buffers made from known statistics in float64
    L, g = 3, torch.Generator().manual_seed(5)
    s, r0 = torch.randn(L, 4, generator=g, dtype=torch.float64), torch.randn(4, generator=g, dtype=torch.float64)
    A = torch.tensor([cc.momentum_weights(m, L)[1] for m in cc.STAT_MOMENTA], dtype=torch.float64)
    for j, m in enumerate(cc.STAT_MOMENTA):      # the module's update, one step per layer
        r, n = r0.clone(), 0
        for l in range(L):
            n += 1
            f = 1.0 / n if m is None else m
            r = (1 - f) * r + f * s[l]
        assert torch.allclose(r, cc.momentum_weights(m, L)[0] * r0 + A[j] @ s, rtol=0, atol=1e-14)


@pytest.mark.parametrize("name", list(cc.CASES))
def test_float32_oracle_is_within_a_tenth_of_the_tolerance(name):
    ref64, ref32 = cc.reference(name, torch.float64), cc.reference(name, torch.float32)
    assert cc.all_finite(ref64) and cc.all_finite(ref32)
    e = cc.errors(ref32, ref64)
    # Gradients that vanish in exact arithmetic whatever the inputs (float64 leaves 1e-17 of the largest gradient norm): the class
    # activation head's bias (a softmax ignores a common shift) and the LAST layer's conv_norms bias (all that follows it are the two
    # BatchNorms, which remove a per-channel constant); at Tc = 1 also what feeds a softmax over one entry.  Their measure is rounding
    # noise over the floor, and no seed or scale moves it (d_logits x 0, x 10, d_masks x 0, x 10: 1.35e-5 .. 1.43e-5 at
    # plain_rate_over_tc), so TOL / 10 cannot be a condition on the inputs there: fp32 torch leaves 1.0e-5 .. 2.1e-5 of the floor on
    # conv_norms.{L-1}.bias over the ten cases and up to 6.7e-6 on the other.  They are recognised from float64 alone, must be exactly
    # this set, and the fp32 noise on them must stay under 1e-7 of the largest gradient norm (a sum of a few thousand fp32 terms of
    # that scale that cancels: some ulps of it).
    scale = max(float(v.norm()) for v in ref64["grads"].values())
    vanishing = sorted("grad." + k for k, v in ref64["grads"].items() if float(v.norm()) < 1e-12 * scale)
    c = cc.CASES[name]
    expect = ["grad._predictor._transformer_class_activation_head.conv.bias", f"grad.conv_norms.{c.layers - 1}.bias"]
    if c.B * c.Tc == 1:       # a softmax over one entry is the constant 1: the activation head's weight has no gradient either
        expect.append("grad._predictor._transformer_class_activation_head.conv.weight")
    if c.Tc == 1:             # and so is the trajectory attention's softmax over one frame, which is all that proj_q feeds
        expect += [f"grad.transformer_trajectory_self_attention_layers.{l}.self_attn.proj_q.{p}" for l in range(c.layers) for p in ("weight", "bias")]
    assert vanishing == sorted(expect)
    for k in vanishing:
        noise = float(ref32["grads"][k[5:]].double().norm()) / scale
        print(f"{name}: {k} vanishes in exact arithmetic, fp32 noise {noise:.2e} of the largest gradient norm")
        assert noise < 1e-7
        del e[k]
    worst = max(e, key=e.get)
    print(f"{name}: fp32 oracle vs float64, worst {worst} {e[worst]:.2e}")
    assert e[worst] < cc.TOL / 10, {k: f"{v:.2e}" for k, v in e.items() if v >= cc.TOL / 10}
    # the gradients under the floor of their measure (1e-3 of the largest norm): besides the two above only proj_q of the trajectory
    # attention, whose gradient is small by construction; in particular no gradient of the mask path (d_masks is scaled by 0.01)
    hidden = sorted(k for k, v in ref64["grads"].items() if float(v.norm()) < 1e-3 * scale and "grad." + k not in vanishing)
    print(f"{name}: gradients under the floor: {hidden}")
    assert all(".self_attn.proj_q." in k for k in hidden), hidden
