"""The finalists of the layout search on the device: every minimum-pass plan `SingleGpuEngine.finalist_plans` returns --
line-qubit triples found by one qsim_plan_search_triples call, placed, priced -- computes the circuit's state, in the
passes the search counted."""
import numpy as np
import pytest

from oracle import dense_oracle as orc

pytestmark = pytest.mark.gpu


def test_every_finalist_plan_against_the_dense_oracle():
    """The 40-layer random 1q + CX circuit at 13 qubits: each finalist plan from |0..0>, compared through its layout."""
    from quantum_simulations_amd.circuit.fusion import batch_levels
    from quantum_simulations_amd.circuit.io import levelize, validate_circuit_dict
    from quantum_simulations_amd.circuits import random_1q_cx_circuit
    from quantum_simulations_amd.runner.engine import SingleGpuEngine, gate_ops
    n = 13
    cd = validate_circuit_dict(random_1q_cx_circuit(n, depth=40))
    want = np.zeros(1 << n, dtype=np.complex128)
    want[0] = 1.0
    orc.apply_ops(want, gate_ops(cd))
    eng = SingleGpuEngine(n, layout="search")
    eng.LAYOUT_MIN_QUBITS = min(n, eng.LAYOUT_MIN_QUBITS)
    try:
        plans = eng.finalist_plans([p["local_ops"] for p in batch_levels(levelize(cd), n)], eng.LAYOUT_FINALISTS)
        assert 1 <= len(plans) <= eng.LAYOUT_FINALISTS
        for plan in plans:
            info = plan.layout_info
            eng.init_zero_state()
            eng.execute(plan)
            err = float(np.max(np.abs(eng.state_vector() - want)))
            print(f"line qubits {info['line_qubits']}: {eng.last_passes} passes ({info['minimum_pass_triples']} of "
                  f"{info['candidates']} candidates reach them), max |device - oracle| {err:.3e}")
            assert eng.last_passes == info["passes_chosen"]
            assert err <= 1e-12
        assert len({p.layout_info["passes_chosen"] for p in plans}) == 1
    finally:
        eng.close()
