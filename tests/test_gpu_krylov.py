"""quantum_simulations_amd.krylov on an MI355X: the cases of tests/test_krylov_cpu.py at 10 and 12 qubits through real
chunks, SingleGpuEngine and single_node, with the same bounds (see there for where they come from), against dense
eigen-decompositions computed once per model and size and shared."""
import numpy as np
import pytest

from quantum_simulations_amd import circuits as gen
from quantum_simulations_amd import evolution, krylov
from quantum_simulations_amd.circuit.staging import permute_state
from quantum_simulations_amd.kernel.device import DeviceChunk
from tests.krylov_reference import (Spectrum, dense_matrix, heisenberg_chain, ising_chain, popcount, rand_state, to_physical_state,
                                    zz_chain)
from tests.rotation_reference import rotate_list
from tests.twostate_reference import apply_sum

pytestmark = pytest.mark.gpu

M, TOL = 16, 1e-8
MODELS = {"ising": ising_chain, "heisenberg": heisenberg_chain}
_SPECTRUM, _E0 = {}, {}


def spectrum(name, n):
    """The full decomposition: the Heisenberg chain conserves the popcount (blocks of at most 924 at n = 12), the Ising
    chain is decomposed whole at n = 10 only."""
    if (name, n) not in _SPECTRUM:
        assert name == "heisenberg" or n <= 10
        _SPECTRUM[name, n] = Spectrum(MODELS[name](n), n, popcount(n) if name == "heisenberg" else None)
    return _SPECTRUM[name, n]


def e0(name, n):
    if (name, n) not in _E0:
        if name == "heisenberg" or n <= 10:
            _E0[name, n] = spectrum(name, n).e0
        else:
            _E0[name, n] = float(np.linalg.eigvalsh(dense_matrix(MODELS[name](n), n).real)[0])
    return _E0[name, n]


def _check_ground_state(result, psi, obs, name, n, what):
    """The bounds of tests/test_krylov_cpu.py::test_ground_state on (energy, residual, restarts, H applications) and the
    final vector in LOGICAL order."""
    energy, residual, restarts, h_apps = result
    true_res = float(np.linalg.norm(apply_sum(psi, obs.x, obs.z, obs.coeffs) - energy * psi))
    print(f"{what} {name} n={n}: E = {energy:.12f} (E_0 = {e0(name, n):.12f}), residual {residual:.3e}, recomputed {true_res:.3e}, "
          f"{restarts} restarts, {h_apps} H applications")
    assert residual <= TOL
    assert true_res <= TOL + 1e-11
    assert abs(energy - e0(name, n)) <= TOL
    assert restarts <= 20
    assert abs(np.linalg.norm(psi) - 1.0) < 1e-13


class Chunks:
    """A state chunk and m work chunks, closed together."""

    def __init__(self, psi, m):
        self.all = []
        try:
            self.all.append(DeviceChunk.from_numpy(psi))
            for _ in range(m):
                self.all.append(DeviceChunk.empty(self.all[0].k))
        except Exception:
            self.close()
            raise
        self.chunk, self.work = self.all[0], self.all[1:]

    def close(self):
        for c in self.all:
            c.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


@pytest.mark.parametrize("reorth", [True, False], ids=["reorth", "plain"])
@pytest.mark.parametrize("n", [10, 12])
@pytest.mark.parametrize("name", list(MODELS))
def test_ground_state(name, n, reorth):
    obs = MODELS[name](n)
    with Chunks(rand_state(n, 3), M) as c:
        result = krylov.ground_state(c.chunk, c.work, None, obs, m=M, tol=TOL, reorth=reorth)
        _check_ground_state(result, c.chunk.download(), obs, name, n, f"chunks reorth={reorth}")
        assert result[3] == result[2] * (M + 1)


@pytest.mark.parametrize("name,n", [("ising", 10), ("heisenberg", 10), ("heisenberg", 12)])
def test_evolve_real_and_imaginary_time(name, n):
    obs, spec = MODELS[name](n), spectrum(name, n)
    psi0 = 0.7 * rand_state(n, 5)
    with Chunks(psi0, M) as c:
        est = krylov.evolve(c.chunk, c.work, None, obs, 0.5, m=M, steps=4)
        got, exact = c.chunk.download(), spec.evolve(psi0, 0.5)
        err, l2 = float(np.max(np.abs(got - exact))), float(np.linalg.norm(got - exact))
        print(f"{name} n={n}: max |got - exact| = {err:.3e} (bound 1e-12), l2 error {l2:.3e}, estimate {est:.3e}")
        assert err < 1e-12
        assert est >= l2
        c.chunk.upload(psi0 / 0.7)
        krylov.evolve(c.chunk, c.work, None, obs, -0.5j, m=M, steps=4)
        got, exact = c.chunk.download(), spec.evolve(psi0 / 0.7, -0.5j)
        assert abs(np.linalg.norm(got) / np.linalg.norm(exact) - 1.0) < 1e-12   # unnormalised: exp(-tau H) psi itself
        err = float(np.max(np.abs(got / np.linalg.norm(got) - exact / np.linalg.norm(exact))))
        print(f"{name} n={n}: imaginary time, max |got - exact| after normalising = {err:.3e} (bound 1e-12)")
        assert err < 1e-12


def test_breakdown_in_an_eigenstate():
    n = 10
    obs = zz_chain(n)
    want = float(np.sum(obs.coeffs))                                              # |0..0>: every Z Z = +1
    start = np.zeros(1 << n)
    start[0] = 2.0
    with Chunks(start, 4) as c:
        alphas, betas, k = krylov.lanczos(c.chunk, c.work, None, obs, 4)
        assert k == 1 and alphas.shape == betas.shape == (1,) and abs(alphas[0] - want) < 1e-14 and betas[0] < 1e-14
        energy, residual, restarts, h_apps = krylov.ground_state(c.chunk, c.work, None, obs, m=4)
        assert abs(energy - want) < 1e-14 and residual < 1e-14 and restarts == 1 and h_apps == 2
        assert np.array_equal(c.chunk.download(), start / 2.0)


@pytest.mark.parametrize("name", list(MODELS))
def test_a_layout_gives_the_same_energies(name):
    n = 10
    l2p = [int(p) for p in np.random.default_rng(7).permutation(n)]
    psi0, obs = rand_state(n, 8), MODELS[name](n)
    with Chunks(psi0, M) as plain, Chunks(to_physical_state(psi0, l2p), M) as moved:
        a0, b0, _ = krylov.lanczos(plain.chunk, plain.work, None, obs, M)
        a1, b1, _ = krylov.lanczos(moved.chunk, moved.work, l2p, obs, M)
        assert np.max(np.abs(a0 - a1)) < 1e-12 and np.max(np.abs(b0 - b1)) < 1e-12
        r0 = krylov.ground_state(plain.chunk, plain.work, None, obs, m=M, tol=TOL)
        r1 = krylov.ground_state(moved.chunk, moved.work, l2p, obs, m=M, tol=TOL)
        assert abs(r0[0] - r1[0]) <= TOL
        _check_ground_state(r1, permute_state(moved.chunk.download(), l2p), obs, name, n, "permuted chunks")


def test_argument_errors_leave_the_chunks_alone():
    n = 6
    psi0, obs = rand_state(n, 9), ising_chain(n)
    with Chunks(psi0, 4) as c:
        small = DeviceChunk.empty(n - 1)
        try:
            for call in (lambda: krylov.ground_state(c.chunk, c.work[:3], None, obs, m=4),
                         lambda: krylov.ground_state(c.chunk, c.work, None, obs, m=1),
                         lambda: krylov.ground_state(c.chunk, [c.chunk] + c.work[:3], None, obs, m=4),
                         lambda: krylov.ground_state(c.chunk, c.work[:3] + [small], None, obs, m=4),
                         lambda: krylov.evolve(c.chunk, c.work, None, obs, 0.1, m=4, steps=0)):
                with pytest.raises(ValueError):
                    call()
            assert c.chunk.download().tobytes() == psi0.tobytes()
            c.chunk.init_zero(False)
            with pytest.raises(ValueError):
                krylov.ground_state(c.chunk, c.work, None, obs, m=4)             # a zero start vector
        finally:
            small.close()


# ---- the engine and the runner ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("staged", [False, True], ids=["identity", "staged"])
def test_engine(staged):
    from quantum_simulations_amd.runner.engine import SingleGpuEngine
    n, name = 12, "heisenberg"
    obs = MODELS[name](n)
    eng = SingleGpuEngine(n, layout="search" if staged else "identity")
    try:
        eng.init_zero_state()
        eng.execute(eng.plan(gen.random_1q_cx_circuit(n, depth=6, seed=9), repeats=8 if staged else 1))
        if staged:
            l2p = [int(p) for p in np.random.default_rng(3).permutation(n)]
            eng._adopt_layout(l2p)                                   # (SWAP passes: the state now lives in that layout)
            assert eng.l2p == l2p
        layout = eng.l2p
        eng.variance(obs)                                            # (allocates the engine's second chunk)
        work, held = eng._work, eng._work.download()
        # evolution first: the state left by `execute` is a generic vector
        psi0 = eng.state_vector()
        est = eng.evolve_krylov(obs, 0.5, m=M, steps=4)
        got, exact = eng.state_vector(), spectrum(name, n).evolve(psi0, 0.5)
        err, l2 = float(np.max(np.abs(got - exact))), float(np.linalg.norm(got - exact))
        print(f"engine staged={staged}: max |got - exact| = {err:.3e} (bound 1e-12), l2 error {l2:.3e}, estimate {est:.3e}")
        assert err < 1e-12 and est >= l2
        assert eng.l2p == layout and not eng._zero                  # the state did not move
        # then the ground state from it; a second call starts from the converged vector and succeeds at once
        result = eng.ground_state(obs, m=M, tol=TOL)
        _check_ground_state(result, eng.state_vector(), obs, name, n, f"engine staged={staged}")
        again = eng.ground_state(obs, m=M, tol=TOL)
        assert again[2] == 1 and again[1] <= TOL and abs(again[0] - e0(name, n)) <= TOL
        assert eng.l2p == layout and not eng._zero
        assert eng._work is work and work.download().tobytes() == held.tobytes()    # `variance`'s chunk is untouched
        with pytest.raises(ValueError):
            eng.ground_state(obs, m=1)
        assert eng.ground_state(obs, m=4, tol=TOL, max_restarts=1)[2] == 1           # the work chunks were released
    finally:
        eng.close()


@pytest.mark.parametrize("staged", [False, True], ids=["identity", "staged"])
def test_single_node(staged):
    from quantum_simulations_amd.runner import single_node
    n = 12
    buf = single_node.run(gen.random_1q_cx_circuit(n, depth=8, seed=5), chunk_size=1 << 9, use_fusion=True, use_staging=staged)
    try:
        l2p = getattr(buf, "log_to_phys", None) or None
        if staged:
            assert l2p and l2p != list(range(n))
        logical = (lambda v: v) if l2p is None else (lambda v: permute_state(v, l2p))
        obs = heisenberg_chain(n)
        held = buf.state.download()
        psi0 = logical(held)
        est = single_node.evolve_krylov(buf, obs, -0.5j, m=M, steps=4)             # imaginary time
        got, exact = logical(buf.state.download()), spectrum("heisenberg", n).evolve(psi0, -0.5j)
        assert abs(np.linalg.norm(got) / np.linalg.norm(exact) - 1.0) < 1e-12 and est >= 0.0
        assert float(np.max(np.abs(got / np.linalg.norm(got) - exact / np.linalg.norm(exact)))) < 1e-12
        for name in MODELS:
            # each from the generic state `run` left (an eigenvector of one model may lie in a symmetry sector of the other)
            buf.state.upload(held)
            result = single_node.ground_state(buf, MODELS[name](n), m=M, tol=TOL)
            _check_ground_state(result, logical(buf.state.download()), MODELS[name](n), name, n, f"single_node staged={staged}")
        assert (getattr(buf, "log_to_phys", None) or None) == l2p
    finally:
        buf.close()


def test_evolve_krylov_against_the_trotter_evolution():
    """A cross-check of conventions (sign of t, no factor 1/2, layout): the project's second-order product formula at
    many steps converges to the same state.  The bound is the Trotter error itself, measured in numpy for this H, t and
    step count against the exact evolution, plus the project's 1e-12 for the rounding of each of the two device runs."""
    from quantum_simulations_amd.runner.engine import SingleGpuEngine
    n, t, steps = 10, 0.2, 40
    obs = ising_chain(n)
    psi0 = rand_state(n, 11)
    exact = spectrum("ising", n).evolve(psi0, t)
    trotter = rotate_list(psi0, *evolution.trotter_rotations(obs, t, steps, 2))
    bound = float(np.max(np.abs(trotter - exact)))
    assert 1e-9 < bound < 1e-3, bound                                             # a real Trotter error, far below a convention error
    a, b = SingleGpuEngine(n, layout="identity"), SingleGpuEngine(n, layout="identity")
    try:
        a.state.upload(psi0)
        b.state.upload(psi0)
        a.evolve(obs, t, steps=steps, order=2)
        b.evolve_krylov(obs, t, m=M, steps=2)
        diff = float(np.max(np.abs(a.state_vector() - b.state_vector())))
        print(f"Trotter (order 2, {steps} steps) against Krylov: max |diff| = {diff:.3e}, Trotter error in numpy {bound:.3e}")
        assert diff <= bound + 2e-12
        assert float(np.max(np.abs(b.state_vector() - exact))) < 1e-12
    finally:
        a.close()
        b.close()
