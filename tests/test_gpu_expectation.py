"""qsim_expectation_pauli on an MI355X against the numpy restatement of <psi|P|psi> (observable.pauli_terms_np) at
1e-12: small random states (3 to 20 qubits, chunks below 256 amplitudes, views), every single-qubit Pauli, random
strings, terms wider than a tile; bitwise-repeatable calls; the pass count; the engine, single_node and dynamic-circuit
paths in staged layouts; closed forms at 30 qubits."""
import ctypes as C

import numpy as np
import pytest

from quantum_simulations_amd import _lib
from quantum_simulations_amd import circuits as gen
from quantum_simulations_amd.circuit.dynamic import validate_dynamic
from quantum_simulations_amd.circuit.import_qasm import qasm_to_dynamic
from quantum_simulations_amd.circuit.staging import permute_state
from quantum_simulations_amd.kernel.device import DeviceChunk, plan_expectation
from quantum_simulations_amd.observable import PauliSum, pauli_terms_np

pytestmark = pytest.mark.gpu


def _rand_state(n, seed):
    rng = np.random.default_rng(seed)
    psi = rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)
    return psi / np.linalg.norm(psi)


def _terms(n, seed):
    """(x, z) masks: every single-qubit X / Y / Z, random strings of weight 1..n, and (n >= 12) strings wider than a tile."""
    rng = np.random.default_rng(seed)
    xs, zs = [0], [0]
    for q in range(n):
        for bx, bz in ((1, 0), (1, 1), (0, 1)):
            xs.append(bx << q)
            zs.append(bz << q)
    for w in range(1, n + 1):
        for _ in range(3):
            x = z = 0
            for q in rng.choice(n, size=w, replace=False):
                bx, bz = ((1, 0), (1, 1), (0, 1))[int(rng.integers(3))]
                x |= bx << int(q)
                z |= bz << int(q)
            xs.append(x)
            zs.append(z)
    if n >= 12:
        full = (1 << n) - 1
        xs += [full, full, full ^ 0b111, (full >> 3) << 3, full & ~1]
        zs += [0, full, 0b101, 1 << (n - 1), (1 << (n - 1)) | 1]
    return np.array(xs, dtype=np.uint64), np.array(zs, dtype=np.uint64)


@pytest.mark.parametrize("n", list(range(3, 21)))
def test_against_numpy(n):
    psi = _rand_state(n, n)
    x, z = _terms(n, 100 + n)
    want = pauli_terms_np(psi, x, z)
    c = DeviceChunk.from_numpy(psi)
    try:
        got = c.expectation_pauli(x, z)
        err = float(np.max(np.abs(got - want)))
        assert err < 1e-12, (n, err, int(np.argmax(np.abs(got - want))))
        assert c.last_expectation_passes == len(plan_expectation(n, x)[1])
        again = c.expectation_pauli(x, z)
        assert got.tobytes() == again.tobytes()                     # bitwise repeatable
        # a term of the same string on its own (another pass plan) agrees too
        solo = c.expectation_pauli(x[-1:], z[-1:])
        assert abs(solo[0] - want[-1]) < 1e-12
        assert c.expectation_pauli([], []).size == 0
    finally:
        c.close()


def test_views():
    psi = _rand_state(14, 5)
    x, z = _terms(10, 6)
    c = DeviceChunk.from_numpy(psi)
    try:
        for off in (0, 3 << 10, 15 << 10):
            v = c.view(off, 10)
            try:
                got = v.expectation_pauli(x, z)
            finally:
                v.close()
            assert float(np.max(np.abs(got - pauli_terms_np(psi[off: off + 1024], x, z)))) < 1e-12
    finally:
        c.close()


def test_nonlocal_bit_fails():
    c = DeviceChunk.from_numpy(_rand_state(8, 1))
    try:
        lib = _lib.load()
        for xm, zm in ((1 << 8, 0), (0, 1 << 9), (1, 1 << 63)):
            x = np.array([1, xm], dtype=np.uint64)
            z = np.array([0, zm], dtype=np.uint64)
            out = np.zeros(2)
            passes = C.c_int(-1)
            rc = lib.qsim_expectation_pauli(c._h, 2, _lib.ptr(x), _lib.ptr(z), _lib.ptr(out), C.byref(passes))
            assert rc == _lib.QSIM_ERR_NONLOCAL
        with pytest.raises(NotImplementedError):
            c.expectation_pauli([1 << 8], [0])
    finally:
        c.close()


def _obs(n, seed):
    rng = np.random.default_rng(seed)
    terms = [(0.5, {0: "X"}), (-0.25, {n - 1: "Y", 0: "Z"}), (1.5, {1: "Z", n - 2: "Z"}), (0.75, {q: "X" for q in range(n)})]
    for _ in range(20):
        qs = rng.choice(n, size=int(rng.integers(1, 6)), replace=False)
        terms.append((float(rng.standard_normal()), {int(q): "XYZ"[int(rng.integers(3))] for q in qs}))
    return PauliSum(terms, n_qubits=n)


def _want(obs, psi_logical):
    return obs.value(pauli_terms_np(psi_logical, *obs.masks()))


def test_engine_in_a_non_identity_layout():
    from quantum_simulations_amd.runner.engine import SingleGpuEngine
    n = 14
    eng = SingleGpuEngine(n, layout="search")
    try:
        cd = gen.random_1q_cx_circuit(n, depth=6, seed=9)
        eng.init_zero_state()
        eng.execute(eng.plan(cd, repeats=8))
        l2p = list(np.random.default_rng(3).permutation(n))
        eng._adopt_layout(l2p)                                   # (SWAP passes: the state now lives in that layout)
        assert eng.l2p == l2p
        obs = _obs(n, 4)
        psi = eng.state_vector()
        before = eng.state.download()
        got = eng.expectation(obs)
        assert abs(got - _want(obs, psi)) < 1e-12
        assert np.array_equal(eng.state.download(), before)      # read-only
    finally:
        eng.close()


def test_single_node_staged():
    from quantum_simulations_amd.runner import single_node
    n = 12
    cd = gen.random_1q_cx_circuit(n, depth=8, seed=5)
    buf = single_node.run(cd, chunk_size=1 << 9, use_fusion=True, use_staging=True)
    try:
        assert buf.log_to_phys and buf.log_to_phys != list(range(n))
        psi = permute_state(buf.state.download(), buf.log_to_phys)
        obs = _obs(n, 7)
        assert abs(single_node.expectation(buf, obs) - _want(obs, psi)) < 1e-12
    finally:
        buf.close()


def test_dynamic_result_state():
    from quantum_simulations_amd.circuits import dynamic_cc_style_qasm
    from quantum_simulations_amd.runner.dynamic import run_dynamic
    prog = validate_dynamic(qasm_to_dynamic(dynamic_cc_style_qasm(12, seed=3)))
    res = run_dynamic(prog, seed=5)
    try:
        psi = res.state.download()
        obs = _obs(12, 8)
        assert abs(res.state.expectation(obs) - _want(obs, psi)) < 1e-12
    finally:
        res.state.close()


def test_closed_forms_30_qubits():
    from quantum_simulations_amd.runner.engine import SingleGpuEngine
    n = 30
    eng = SingleGpuEngine(n)
    try:
        eng.init_zero_state()
        eng.execute(eng.plan(gen.generate_ghz_circuit(n)))
        ghz = PauliSum({"Z0 Z29": 1.0, "Z3 Z17": 1.0, " ".join(f"X{q}" for q in range(n)): 1.0, "Z5": 1.0, "Z0": 1.0},
                       n_qubits=n)
        x, z = ghz.masks(eng.l2p)
        vals = eng.state.expectation_pauli(x, z)
        assert float(np.max(np.abs(vals - [1.0, 1.0, 1.0, 0.0, 0.0]))) < 1e-12, vals
        theta = np.random.default_rng(30).uniform(0, np.pi, n)
        eng.init_zero_state()
        cd = {"number_of_qubits": n, "gates": [{"qubits": [q], "gate": "RY", "params": {"theta": float(theta[q])}}
                                               for q in range(n)]}
        eng.execute(eng.plan(cd))
        qs = [0, 1, 2, 3, 11, 12, 20, 29]
        terms = [(1.0, {q: "Z"}) for q in qs] + [(1.0, {q: "Y"}) for q in qs]
        terms += [(1.0, {a: "X", b: "X"}) for a, b in ((0, 1), (2, 29), (11, 20), (5, 28))]
        prod = PauliSum(terms, n_qubits=n)
        want = [np.cos(theta[q]) for q in qs] + [0.0] * len(qs)
        want += [np.sin(theta[a]) * np.sin(theta[b]) for a, b in ((0, 1), (2, 29), (11, 20), (5, 28))]
        x, z = prod.masks(eng.l2p)
        vals = eng.state.expectation_pauli(x, z)
        assert float(np.max(np.abs(vals - want))) < 1e-12, vals - want
        assert abs(eng.expectation(prod) - float(np.sum(want))) < 1e-11
    finally:
        eng.close()
