"""GPU: every kernel form the inference planner can choose (tests/infer_plan_cases.py) -- the stages the library runs are the recorded
ones, the output holds the 1e-3 bar against the float64 oracle, and a second call gives the same bits."""
import pytest
import torch

import __graft_entry__ as ge
import infer_plan_cases as ipc
from golden_util import rel_err, rel_l2

pytestmark = pytest.mark.gpu
TOL_F16 = 1e-3      # the bar of test_hip_parity.py


@pytest.fixture(scope="module", autouse=True)
def built():
    ge.build()
    assert torch.cuda.is_available()


@pytest.mark.parametrize("name", list(ipc.CASES))
def test_planned_form_runs_and_holds_the_bar(name):
    outs, names = ipc.run(name)
    again, _ = ipc.run(name)
    ref = ipc.reference(name)
    out = outs["out"].double().cpu()
    e, e2 = rel_err(out, ref), rel_l2(out, ref)
    print(f"{name}: {names} max/max {e:.2e} relL2 {e2:.2e}")
    assert names == ipc.STAGES[name], (names, ipc.STAGES[name])
    assert e < TOL_F16 and e2 < TOL_F16
    assert all(torch.equal(v, again[k]) for k, v in outs.items())
