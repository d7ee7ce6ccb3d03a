"""The priced planner on the device: plans of SingleGpuEngine(layout="search") with the engine pricing on -- rule (d) of
the op rewrite and the placement of the ops that need no tile (runner/engine.py `priced_variant`, executed through
`qsim_apply_ops_placed`, which is also handed placements directly) -- against the C oracle at the smallest size the searching branch runs at, and at 24 qubits (two
tiles per workgroup) by the layout-aware fingerprint against an identity-layout plan of the circuit's own ops, as
bench.py's `timed_plan_check`."""
import numpy as np
import pytest

from oracle import c_oracle
from quantum_simulations_amd import circuits as gen
from quantum_simulations_amd.circuit.io import validate_circuit_dict

pytestmark = pytest.mark.gpu

TOL = 1e-12                        # amplitudes against the C oracle (the issue's bound)
FINGERPRINT_TOL = 1e-10            # bench.py's PARITY_TOL for the timed plan's fingerprint (the issue's bound)


def _engine(n, candidates):
    from quantum_simulations_amd.runner.engine import SingleGpuEngine
    eng = SingleGpuEngine(n, layout="search")
    eng.LAYOUT_MIN_QUBITS = min(n, eng.LAYOUT_MIN_QUBITS)        # (the search is for >= 26 qubits by default)
    eng.LAYOUT_CANDIDATES = candidates
    assert eng.ENGINE_PRICING
    return eng


@pytest.mark.parametrize("name", ["random", "clifford_t"])
def test_priced_search_plans_equal_the_c_oracle(name):
    n = 12                         # the smallest size with a choice of tile: the searching branch plans nothing smaller differently
    cd = (gen.random_1q_cx_circuit(n, depth=20, seed=350 + n) if name == "random"
          else gen.random_clifford_t_circuit(n, depth=40, seed=360 + n))
    eng = _engine(n, 8)
    eng.init_zero_state()
    plan = eng.plan(cd)
    info = plan.layout_info
    split = info["model_split_ms"]
    print(name, {k: v for k, v in info.items() if k in ("passes_chosen", "model_split_ms", "rewrite")})
    assert split["passes"] <= split["passes_unpriced"]
    eng.execute(plan)
    assert eng.last_passes == info["passes_chosen"], name             # the library took the named tiles and the placement
    np.testing.assert_allclose(eng.state_vector(), c_oracle.simulate(validate_circuit_dict(cd)), rtol=0, atol=TOL, err_msg=name)
    eng.close()


@pytest.mark.parametrize("n", [12, 14])
def test_placements_run_on_the_device(n):
    """`qsim_apply_ops_placed` itself: the placement `planner.balance` makes when every second pass has room, and one
    drawn at random, on a list with identities in it (they drop out of the planned list: the placement is indexed by the
    caller's ops) -- the oracle's state from a random start, the planner's pass count, the same again from the plan cache,
    and the tiles without a placement next to it (another cache entry)."""
    from oracle import dense_oracle
    from quantum_simulations_amd.kernel import planner
    from quantum_simulations_amd.kernel.device import DeviceChunk
    from quantum_simulations_amd.runner import engine_cost
    from tests.test_gpu_kernels import _rand_state
    from tests.test_op_rewrite_cpu import device_cases
    costs = engine_cost.table()
    ops = planner.rewrite_ops(n, device_cases(n)[0][2])
    eye = np.eye(2, dtype=np.complex128)
    ops = ops[:7] + [([3], eye)] + ops[7:40] + [([n - 1], eye)] + ops[40:]
    masks = planner.search_tiles(n, ops)
    mem = np.where(np.arange(len(masks)) % 2 == 0, 0.0, 1e9)
    balanced, before, after = planner.balance(n, ops, masks, mem, costs)
    assert (balanced > 0).sum() > 0 and np.maximum(mem, after).sum() < np.maximum(mem, before).sum()
    drawn = np.random.default_rng(n).integers(0, len(masks) + 1, size=len(ops)).astype(np.int32)
    dev = DeviceChunk.empty(n)
    for name, place in (("balanced", balanced), ("drawn", drawn)):
        want_passes = planner.pass_count(n, ops, masks, place)
        for again in range(2):
            psi = _rand_state(n, 60 + n)
            want = psi.copy()
            dense_oracle.apply_ops(want, ops)
            dev.upload(psi)
            assert dev.apply_ops_placed(ops, masks, place) == want_passes, (name, again)
            np.testing.assert_allclose(dev.download(), want, rtol=0, atol=TOL, err_msg=f"{name} {again}")
        dev.upload(psi)
        assert dev.apply_ops_tiled(ops, masks) == len(masks), name
        np.testing.assert_allclose(dev.download(), want, rtol=0, atol=TOL, err_msg=f"{name} tiled")
    with pytest.raises(ValueError):
        dev.apply_ops_placed(ops, masks, balanced[:-1])
    dev.close()


def test_priced_plan_fingerprint_at_two_tiles_per_workgroup():
    """24 qubits: 2 x 4096 tiles, so every workgroup of a pass takes two (the shape of test_gpu_engine_cases_paired.py)"""
    from quantum_simulations_amd.kernel import planner
    n, seed = 24, 20260504
    assert planner.tiles_per_workgroup(n, 11) == 2
    cd = gen.random_1q_cx_circuit(n, depth=24, seed=24)
    eng = _engine(n, 8)
    eng.init_zero_state()
    plan = eng.plan(cd)
    split = plan.layout_info["model_split_ms"]
    print({k: v for k, v in plan.layout_info.items() if k in ("passes_chosen", "model_split_ms", "rewrite")})
    assert split["rule_d_ops"] > 0                                    # (a depth-24 random circuit has diagonals next to dense gates)
    eng.execute(plan)
    assert eng.last_passes == plan.layout_info["passes_chosen"]
    fp_priced = eng.state.fingerprint(n, 0, eng.l2p, seed)
    eng.layout_mode = "identity"                                      # index bit = qubit, the circuit's own ops, the library's own tiles
    eng.init_zero_state()
    plain = eng.plan(cd, repeats=1)
    eng.execute(plain)
    fp_plain = eng.state.fingerprint(n, 0, eng.l2p, seed)
    norm2 = eng.norm2()
    eng.close()
    print(f"fingerprints {abs(fp_priced - fp_plain):.3e} apart; norm2 {norm2:.15f}")
    assert abs(fp_priced - fp_plain) < FINGERPRINT_TOL
    assert abs(norm2 - 1.0) < 1e-12
