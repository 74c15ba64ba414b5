"""GPU: the inference tier's trajectory kernels at large and at almost one-hot softmax logits (tests/infer_regime_cases.py: the regimes
shift, sharp_s and sharp_t on cases of infer_plan_cases.py, screened on the CPU) -- one eval forward per (case, regime) with the regime's
weights loaded, through the runner of infer_plan_cases.

Per pair: the stage names are the recorded ones of the case (the kernel form under test ran); every output is finite and within
max(1e-3, 2 x yardstick) of the float64 oracle, the yardstick being tests/f16_sites.py -- the layer with the kernels' fp16 roundings, in
float64 -- at the pair's multipliers over four weight seeds; the attention maps of maps_temporal_fused sum to 1 per row and lie within
max(3e-3, 2 x the yardstick's own map error); a second forward gives the same bits; and the weights as drawn at the pair's seed hold the
standing 1e-3 bar.  profiles/infer_regimes_parity.txt is the printed line per pair and tensor from an MI355X."""
import pytest
import torch

import __graft_entry__ as ge
import infer_plan_cases as ipc
import infer_regime_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def built():
    ge.build()
    assert torch.cuda.is_available()


@pytest.mark.parametrize("name,regime", rc.pair_ids())
def test_regime_forward_vs_float64_oracle(name, regime):
    w = rc.pair_weights(name, regime)
    outs, names = ipc.run(name, w)
    again, _ = ipc.run(name, w)
    assert names == ipc.STAGES[name], (names, ipc.STAGES[name])
    got = {k: v.float().cpu() for k, v in outs.items()}
    lines = []
    misses = rc.missed(name, regime, got, lines, rc.tag(name, regime))
    print("\n".join(lines))
    assert not misses, misses
    assert all(torch.equal(v, again[k]) for k, v in outs.items())
    base, names = ipc.run(name, rc.pair_weights(name, regime, plain_weights=True))
    assert names == ipc.STAGES[name]
    misses = rc.plain_missed(name, regime, {k: v.float().cpu() for k, v in base.items()})
    assert not misses, misses
