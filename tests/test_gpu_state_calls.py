"""`state_calls.StateCalls` through its two front doors on an MI355X: `SingleGpuEngine` and `HbmStateBuffer`
(`single_node`'s module functions).  n = 10, Krylov m = 3.

1. The engine must know that a call wrote the state: after each mutating call from |0..0> a plan written for ANOTHER
   layout is executed, and the state must have been moved there by SWAPs, not relabelled (|0..0> alone may be).
2. Both front doors give the same numbers on the same state in the same staging layout, and the buffer closes every
   chunk it opens.

Bound 1e-11 absolute on unit-norm states, the bound of the feature tests of these calls through the engines
(tests/test_gpu_diagonal.py, test_gpu_hamiltonian.py, test_gpu_krylov.py): every call here is at most a few hundred
passes whose rounding is a few 2.2e-16 each.  The numpy references are the ones the feature tests use; for the two Krylov
calls the same `krylov` module on the host chunk of tests/diagonal_operator_reference.py (three Lanczos steps and a 3 x 3
eigenproblem: a short, well-conditioned computation)."""
import numpy as np
import pytest

from quantum_simulations_amd import circuits as gen
from quantum_simulations_amd import diagonal, evolution, krylov
from quantum_simulations_amd.circuit.staging import permute_state
from quantum_simulations_amd.kernel import gates as gate_table
from quantum_simulations_amd.kernel.device import DeviceChunk, pack_ops
from quantum_simulations_amd.observable import PauliSum
from quantum_simulations_amd.runner import single_node
from quantum_simulations_amd.runner.engine import GpuPlan, SingleGpuEngine
from tests import diagonal_reference as ref
from tests.diagonal_operator_reference import HostChunk
from tests.krylov_reference import ising_chain
from tests.rotation_reference import rotate_list

pytestmark = pytest.mark.gpu

N, M, ATOL = 10, 3, 1e-11
LAYOUT_A = [int(p) for p in np.random.default_rng(3).permutation(N)]
LAYOUT_B = [int(p) for p in np.random.default_rng(4).permutation(N)]
H = ising_chain(N)                                                             # -sum Z Z - 1.5 sum X
D = PauliSum([(0.5 + 0.1 * q, {q: "Z", (q + 3) % N: "Z"}) for q in range(N)] + [(0.3, {0: "Z"}), (-0.7, {4: "Z"})], n_qubits=N)
ROT = [("X0 Z1", 0.3), ("Y2 X7", -0.7), ("Z0 X3", 0.45), ("Y9", 1.1), ("X4 Y5 Z6", -0.2)]
GAMMAS, BETAS = [0.4, -0.9], [0.7, 0.2]
GATE_QUBIT = 6


def _qaoa_np(psi):
    z, co = diagonal.diagonal_part(D)
    for g, b in zip(GAMMAS, BETAS):
        psi = rotate_list(ref.phase(psi, z, co, g), [1 << q for q in range(N)], [0] * N, [b] * N)
    return psi


def _krylov_np(call):
    def run(psi):
        chunk, work = HostChunk(psi), [HostChunk(np.zeros(1 << N)) for _ in range(M)]
        call(chunk, work)
        return chunk.psi
    return run


def _rotations_np(psi):
    x, z, th = evolution.as_rotation_arrays(ROT)
    return rotate_list(psi, x, z, th)


# name -> (the call on an engine, the state it leaves in numpy)
MUTATING = {
    "apply_pauli_rotations": (lambda e: e.apply_pauli_rotations(ROT), _rotations_np),
    "evolve": (lambda e: e.evolve(H, 0.3, steps=2, order=2), lambda psi: rotate_list(psi, *evolution.trotter_rotations(H, 0.3, 2, 2))),
    "apply_diagonal_phase": (lambda e: e.apply_diagonal_phase(D, 0.6), lambda psi: ref.phase(psi, *diagonal.diagonal_part(D), 0.6)),
    "qaoa": (lambda e: e.qaoa(D, GAMMAS, BETAS), _qaoa_np),
    "qaoa_gradient": (lambda e: e.qaoa_gradient(D, GAMMAS, BETAS), lambda psi: psi),
    "gradient": (lambda e: e.gradient(ROT, H), lambda psi: psi),
    "ground_state": (lambda e: e.ground_state(H, m=M, max_restarts=2),
                     _krylov_np(lambda c, w: krylov.ground_state(c, w, None, H, M, 1e-8, 2))),
    "evolve_krylov": (lambda e: e.evolve_krylov(H, 0.2, m=M, steps=2), _krylov_np(lambda c, w: krylov.evolve(c, w, None, H, 0.2, M, 2))),
}
READ_ONLY = {
    "expectation": lambda e: e.expectation(H),
    "diagonal_moments": lambda e: e.diagonal_moments(D),
    "variance": lambda e: e.variance(H),
    "apply_observable": lambda e: e.apply_observable(H),
    "overlap_with": lambda e: e.overlap_with(e.apply_observable(H), H),
    "reduced_density_matrix": lambda e: e.reduced_density_matrix([1, 8]),
    "sample": lambda e: e.sample(64, 5),
}


def _one_gate_plan(l2p) -> GpuPlan:
    """H on logical qubit GATE_QUBIT, written for the layout l2p."""
    plan = GpuPlan([pack_ops([([l2p[GATE_QUBIT]], gate_table.H())])])
    plan.tiles, plan.l2p = [None], l2p
    return plan


def _apply_h(psi):
    out = psi.reshape(1 << (N - 1 - GATE_QUBIT), 2, 1 << GATE_QUBIT)
    return (np.stack([out[:, 0] + out[:, 1], out[:, 0] - out[:, 1]], axis=1) / np.sqrt(2.0)).reshape(-1)


@pytest.mark.parametrize("name", list(MUTATING))
def test_a_written_state_is_moved_not_relabelled(name):
    call, numpy_call = MUTATING[name]
    zero = np.zeros(1 << N, dtype=np.complex128)
    zero[0] = 1.0
    eng = SingleGpuEngine(N, layout="identity")
    try:
        eng.init_zero_state()
        eng._adopt_layout(LAYOUT_A)                                  # |0..0>: relabelled
        assert eng.l2p == LAYOUT_A and eng._zero
        call(eng)
        assert eng.l2p == LAYOUT_A and not eng._zero, name
        eng.execute(_one_gate_plan(LAYOUT_B))
        assert eng.l2p == LAYOUT_B
        err = float(np.max(np.abs(eng.state_vector() - _apply_h(numpy_call(zero)))))
        print(f"{name} from |0..0> in one layout, then a gate planned for another: max |got - want| = {err:.3e} (bound {ATOL:g})")
        assert err < ATOL, name
    finally:
        eng.close()


@pytest.mark.parametrize("name", list(READ_ONLY))
def test_a_read_leaves_the_state_and_what_the_engine_knows_of_it(name):
    eng = SingleGpuEngine(N, layout="identity")
    try:
        eng.init_zero_state()
        eng._adopt_layout(LAYOUT_A)
        READ_ONLY[name](eng)
        assert eng._zero and eng.l2p == LAYOUT_A, name               # |0..0> is still known to be |0..0>
        eng.init_random_state(7)
        eng._adopt_layout(LAYOUT_A)                                  # (SWAP passes: the state now lives in that layout)
        psi = eng.state_vector()
        READ_ONLY[name](eng)
        assert not eng._zero and eng.l2p == LAYOUT_A, name
        eng.execute(_one_gate_plan(LAYOUT_B))
        err = float(np.max(np.abs(eng.state_vector() - _apply_h(psi))))
        print(f"{name} on a random state, then a gate planned for another layout: max |got - want| = {err:.3e} (bound {ATOL:g})")
        assert eng.l2p == LAYOUT_B and err < ATOL, name
    finally:
        eng.close()


def _close_to(a, b) -> float:
    flat = lambda r: np.concatenate([np.asarray(p, dtype=np.complex128).reshape(-1) for p in (r if isinstance(r, tuple) else (r,))])
    return float(np.max(np.abs(flat(a) - flat(b))))


def test_both_front_doors_give_the_same_numbers_and_the_buffer_leaves_no_chunk_open(monkeypatch):
    cd = gen.random_1q_cx_circuit(N, depth=8, seed=6)         # (staged at chunks of 2^8: six qubits change places)
    opened, closed = [], []
    empty, close = DeviceChunk.empty.__func__, DeviceChunk.close

    def counting_empty(cls, k, device=0):
        opened.append(empty(cls, k, device))
        return opened[-1]

    def counting_close(self):
        if self._h is not None and self._h.value and any(self is c for c in opened):
            closed.append(self)
        close(self)
    buf = single_node.run(cd, chunk_size=1 << 8, use_fusion=True, use_staging=True)
    eng = SingleGpuEngine(N, layout="identity")
    spare_b, spare_e = DeviceChunk.empty(N), DeviceChunk.empty(N)
    monkeypatch.setattr(DeviceChunk, "empty", classmethod(counting_empty))
    monkeypatch.setattr(DeviceChunk, "close", counting_close)
    try:
        l2p = buf.l2p
        assert l2p == buf.log_to_phys and sorted(l2p) == list(range(N)) and l2p != list(range(N))
        eng.init_zero_state()
        eng.execute(eng.plan(cd))
        eng._adopt_layout(l2p)                                       # the same vector in the same layout behind both doors
        assert float(np.max(np.abs(eng.state.download() - buf.state.download()))) < ATOL

        def through_buffer(call, *args, **kw):
            before = len(opened), len(closed)
            out = call(*args, **kw)
            assert len(opened) - before[0] == len(closed) - before[1], call                # nothing is left open ...
            assert all(not c._h.value for c in opened[before[0]:]), call
            return out, len(opened) - before[0]

        # read-only calls first, then the calls that write: both states take the same steps
        steps = [("expectation", (H,), {}, 0), ("diagonal_moments", (D,), {}, 0), ("variance", (H,), {"fuse_diagonal": True}, 1),
                 ("reduced_density_matrix", ([1, 8, 3],), {}, 0), ("sample", (64, 5, [0, 2, 9]), {}, 0),
                 ("evolve", (H, 0.3), {"steps": 2, "order": 2}, 0), ("apply_diagonal_phase", (D, 0.6), {}, 0),
                 ("qaoa", (D, GAMMAS, BETAS), {}, 0), ("qaoa_gradient", (D, GAMMAS, BETAS), {}, 1), ("gradient", (ROT, H), {}, 1),
                 ("evolve_krylov", (H, 0.2), {"m": M, "steps": 2}, M), ("ground_state", (H,), {"m": M, "max_restarts": 2}, M)]
        assert len(steps) == 12
        for name, args, kw, chunks in steps:
            got, n_opened = through_buffer(getattr(single_node, name), buf, *args, **kw)
            want = getattr(eng, name)(*args, **kw)
            err = _close_to(got, want)
            print(f"{name}: |single_node - engine| = {err:.3e} (bound {ATOL:g}); the buffer opened and closed {n_opened} chunks")
            assert err < ATOL and n_opened == chunks, name
        # the three calls without a module function, through the buffer's methods
        got, _ = through_buffer(buf.apply_pauli_rotations, ROT)
        assert got == eng.apply_pauli_rotations(ROT)
        out_b, n_opened = through_buffer(buf.apply_observable, H, out=spare_b)
        assert out_b is spare_b and n_opened == 0
        err = float(np.max(np.abs(spare_b.download() - eng.apply_observable(H, out=spare_e).download())))
        got, _ = through_buffer(buf.overlap_with, spare_b, H)
        err = max(err, abs(got - eng.overlap_with(spare_e, H)), abs(buf.overlap_with(spare_b) - eng.overlap_with(spare_e)))
        print(f"apply_observable / overlap_with: |buffer - engine| = {err:.3e} (bound {ATOL:g})")
        assert err < ATOL
        before = len(opened), len(closed)
        with pytest.raises(ValueError, match="at least 2"):
            single_node.ground_state(buf, H, m=1)                    # ... nor when the call raises
        assert (len(opened) - before[0], len(closed) - before[1]) == (1, 1)
        assert all(not c._h.value for c in opened if c is not eng._work)
        # the states behind both doors are still the same vector, in the layout they started in
        assert buf.l2p == l2p and eng.l2p == l2p
        err = float(np.max(np.abs(permute_state(buf.state.download(), l2p) - eng.state_vector())))
        print(f"final states: max |single_node - engine| = {err:.3e} (bound {ATOL:g})")
        assert err < ATOL and abs(eng.norm2() - 1.0) < ATOL
    finally:
        monkeypatch.undo()
        for c in (spare_b, spare_e):
            c.close()
        eng.close()
        buf.close()
