"""The op-list rewrite on the device: plans made by SingleGpuEngine(layout="search") are planned from the rewritten
batches (csrc/op_rewrite.h) -- their state against the oracle's state of the ORIGINAL circuit, amplitude by amplitude,
from |0..0> and from a random state (a wrongly flushed X at the front of the list is invisible on |0..0> only by luck)."""
import numpy as np
import pytest

from oracle import c_oracle, dense_oracle
from quantum_simulations_amd.circuit.io import validate_circuit_dict
from tests.test_op_rewrite_cpu import device_cases

pytestmark = pytest.mark.gpu

TOL = 1e-12


def _engine(n, candidates):
    from quantum_simulations_amd.runner.engine import SingleGpuEngine
    eng = SingleGpuEngine(n, layout="search")
    eng.LAYOUT_MIN_QUBITS = min(n, eng.LAYOUT_MIN_QUBITS)        # (the search is for >= 26 qubits by default)
    eng.LAYOUT_CANDIDATES = candidates
    return eng


@pytest.mark.parametrize("start", ["zero", "random"])
@pytest.mark.parametrize("n", [12, 14])       # 12: the smallest size with a choice of tile and the full 2^11 engine text
def test_rewritten_plans_equal_the_oracle_of_the_original_circuit(n, start):
    eng = _engine(n, 8)
    for name, cd, ops in device_cases(n):
        if start == "zero":
            eng.init_zero_state()
            psi0 = np.zeros(1 << n, dtype=np.complex128)
            psi0[0] = 1.0
        else:
            eng.init_random_state(40 + n)
            psi0 = eng.state_vector()
        plan = eng.plan(cd) if cd is not None else eng.plan_batches([ops])
        info = plan.layout_info
        rewrite = info["rewrite"]
        assert rewrite["ops_in"] == len(ops) and rewrite["need_tile_out"] <= rewrite["need_tile_in"], (name, rewrite)
        assert rewrite["need_tile_out"] < rewrite["need_tile_in"], (name, rewrite)      # (these circuits have X / Y gates to lose)
        if cd is not None and start == "zero":
            want = c_oracle.simulate(validate_circuit_dict(cd))
        else:
            want = psi0.copy()
            dense_oracle.apply_ops(want, ops)
        eng.execute(plan)
        assert eng.last_passes == info["passes_chosen"], name         # the library took the named tiles: no pass more
        np.testing.assert_allclose(eng.state_vector(), want, rtol=0, atol=TOL, err_msg=f"{name} from {start}")
    eng.close()
