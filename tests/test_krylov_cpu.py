"""No GPU: quantum_simulations_amd.krylov -- host bookkeeping over three chunk calls -- driven through the numpy stand-in
chunk of tests/krylov_reference.py, against dense eigen-decompositions of the same Pauli sums.

Bounds.  ground_state: the solver's own stopping rule is the true residual |H psi - E psi| <= tol, and for a normalised
psi |E - E_0| <= residual (E is a Rayleigh quotient: its error is even quadratic in it), so tol bounds both; the residual
recomputed in numpy from the final vector may differ from the solver's by rounding of a 2^10-term sum of O(10) terms,
1e-11 covers that.  evolve: the Krylov truncation error at dt = 0.125, m = 16 is below 1e-15 for these spectra (widths
< 30: (dt * width / 4)^16 / 16! < 1e-15), what remains is rounding of a few hundred passes, each a few 1e-16: 1e-12."""
import numpy as np
import pytest

from quantum_simulations_amd import krylov
from quantum_simulations_amd.observable import PauliSum
from tests.krylov_reference import (HostChunk, dense_matrix, heisenberg_chain, ising_chain, lincomb, rand_state, to_physical_state,
                                    zz_chain)

N, M, TOL = 10, 16, 1e-8
MODELS = {"ising": ising_chain, "heisenberg": heisenberg_chain}
_EIG = {}


def eig(name, n=N):
    """(H, eigenvalues, eigenvectors) of a model, computed once and shared."""
    if (name, n) not in _EIG:
        H = dense_matrix(MODELS[name](n), n)
        _EIG[name, n] = (H,) + tuple(np.linalg.eigh(H))
    return _EIG[name, n]


def chunks(psi, m):
    return HostChunk(psi), [HostChunk(np.zeros(psi.size)) for _ in range(m)]


def test_lincomb_reference():
    rng = np.random.default_rng(1)
    d, s0, s1, b = (rng.standard_normal(8) + 1j * rng.standard_normal(8) for _ in range(4))
    new, dots, n2 = lincomb(d, 0.5 - 2j, [s0, s1], [1j, -0.25], [b, s0], True)
    want = (0.5 - 2j) * d + 1j * s0 - 0.25 * s1
    assert np.allclose(new, want, atol=1e-15) and np.allclose(dots, [np.vdot(b, want), np.vdot(s0, want)], atol=1e-14)
    assert abs(n2 - np.vdot(want, want).real) < 1e-14
    nan = np.full(8, np.nan + 0j)
    assert np.array_equal(lincomb(nan, 0.0, [s0], [2.0])[0], 2.0 * s0)          # dst is not read
    assert not np.any(lincomb(nan, 0.0)[0]) and lincomb(d, 1.0)[2] is None


@pytest.mark.parametrize("reorth", [True, False], ids=["reorth", "plain"])
@pytest.mark.parametrize("name", list(MODELS))
def test_ground_state(name, reorth):
    H, lam, _ = eig(name)
    chunk, work = chunks(rand_state(N, 3), M)
    energy, residual, restarts, h_apps = krylov.ground_state(chunk, work, None, MODELS[name](N), m=M, tol=TOL, reorth=reorth)
    psi = chunk.psi
    true_res = float(np.linalg.norm(H @ psi - energy * psi))
    print(f"{name} reorth={reorth}: E = {energy:.12f} (E_0 = {lam[0]:.12f}, gap {lam[1] - lam[0]:.3f}), residual {residual:.3e}, "
          f"recomputed {true_res:.3e}, {restarts} restarts, {h_apps} H applications")
    assert residual <= TOL
    assert true_res <= TOL + 1e-11
    assert abs(energy - lam[0]) <= TOL
    assert restarts <= 20 and h_apps == restarts * (M + 1)
    assert abs(np.linalg.norm(psi) - 1.0) < 1e-14
    assert lam[1] - lam[0] > 1.0                                                 # a unique ground state


@pytest.mark.parametrize("name", list(MODELS))
def test_lanczos_matrix(name):
    """The tridiagonal matrix is V^+ H V, the vectors are orthonormal, and H V = V T + beta_m v_m e_m^T."""
    H, _, _ = eig(name)
    m = 12
    chunk, work = chunks(3.0 * rand_state(N, 4), m)                              # any norm: normalised in place
    alphas, betas, k = krylov.lanczos(chunk, work, None, MODELS[name](N), m)
    assert k == m and alphas.shape == betas.shape == (m,)
    V = np.stack([chunk.psi] + [w.psi for w in work[:m - 1]], axis=1)
    T = np.diag(alphas) + np.diag(betas[:-1], 1) + np.diag(betas[:-1], -1)
    assert np.max(np.abs(V.conj().T @ V - np.eye(m))) < 1e-13
    assert np.max(np.abs(V.conj().T @ H @ V - T)) < 1e-12
    rest = H @ V - V @ T
    rest[:, -1] -= betas[-1] * work[m - 1].psi
    assert np.max(np.abs(rest)) < 1e-12
    # one H per step, the first step without the beta term, every step normalised by a source-less pass
    assert [c for c in work[0].calls if c[0] == "sum"] == [("sum", len(MODELS[name](N)))]
    assert work[0].calls[1] == ("lincomb", 0, 1, False) and work[1].calls[1] == ("lincomb", 1, 1, False)
    assert work[1].calls[-1] == ("lincomb", 0, 0, False)


@pytest.mark.parametrize("name", list(MODELS))
def test_evolve_real_time(name):
    H, lam, U = eig(name)
    psi0 = 0.7 * rand_state(N, 5)                                                # the norm is carried through
    chunk, work = chunks(psi0, M)
    est = krylov.evolve(chunk, work, None, MODELS[name](N), 0.5, m=M, steps=4)
    exact = U @ (np.exp(-0.5j * lam) * (U.conj().T @ psi0))
    err, l2 = float(np.max(np.abs(chunk.psi - exact))), float(np.linalg.norm(chunk.psi - exact))
    print(f"{name}: max |got - exact| = {err:.3e} (bound 1e-12), l2 error {l2:.3e}, estimate {est:.3e}")
    assert err < 1e-12
    assert est >= l2
    assert abs(np.linalg.norm(chunk.psi) - 0.7) < 1e-13


@pytest.mark.parametrize("name", list(MODELS))
def test_evolve_imaginary_time(name):
    H, lam, U = eig(name)
    psi0 = rand_state(N, 6)
    chunk, work = chunks(psi0, M)
    krylov.evolve(chunk, work, None, MODELS[name](N), -0.5j, m=M, steps=4)
    exact = U @ (np.exp(-0.5 * lam) * (U.conj().T @ psi0))
    assert abs(np.linalg.norm(chunk.psi) / np.linalg.norm(exact) - 1.0) < 1e-12  # unnormalised: exp(-tau H) psi itself
    err = float(np.max(np.abs(chunk.psi / np.linalg.norm(chunk.psi) - exact / np.linalg.norm(exact))))
    print(f"{name}: imaginary time, max |got - exact| after normalising = {err:.3e} (bound 1e-12)")
    assert err < 1e-12


def test_breakdown_in_an_eigenstate():
    n = 8
    obs = zz_chain(n)
    e0 = float(np.sum(obs.coeffs))                                               # |0..0>: every Z Z = +1
    basis0 = np.zeros(1 << n)
    basis0[0] = 2.0
    chunk, work = chunks(basis0, 4)
    alphas, betas, k = krylov.lanczos(chunk, work, None, obs, 4)
    assert k == 1 and alphas.shape == betas.shape == (1,) and alphas[0] == e0 and betas[0] == 0.0
    energy, residual, restarts, h_apps = krylov.ground_state(chunk, work, None, obs, m=4)
    assert energy == e0 and residual == 0.0 and restarts == 1 and h_apps == 2
    assert np.array_equal(chunk.psi, basis0 / 2.0)
    est = krylov.evolve(chunk, work, None, obs, 0.3, m=4, steps=2)
    assert est < 1e-15                                                           # (the second step starts from a rounded phase)
    assert abs(chunk.psi[0] - np.exp(-0.3j * e0)) < 1e-15 and not np.any(chunk.psi[1:])


@pytest.mark.parametrize("name", list(MODELS))
def test_a_layout_gives_the_same_energies(name):
    l2p = [int(p) for p in np.random.default_rng(7).permutation(N)]
    psi0 = rand_state(N, 8)
    obs = MODELS[name](N)
    plain, work = chunks(psi0, M)
    moved, work2 = chunks(to_physical_state(psi0, l2p), M)
    a0, b0, _ = krylov.lanczos(plain, work, None, obs, M)
    a1, b1, _ = krylov.lanczos(moved, work2, l2p, obs, M)
    assert np.max(np.abs(a0 - a1)) < 1e-12 and np.max(np.abs(b0 - b1)) < 1e-12
    e0 = krylov.ground_state(plain, work, None, obs, m=M, tol=TOL)
    e1 = krylov.ground_state(moved, work2, l2p, obs, m=M, tol=TOL)
    assert abs(e0[0] - e1[0]) <= TOL and e0[2] == e1[2]
    assert np.max(np.abs(moved.psi - to_physical_state(plain.psi, l2p))) < 1e-6  # the same vector, moved (phase included)


def test_argument_errors():
    n = 4
    obs = ising_chain(n)
    chunk, work = chunks(rand_state(n, 9), 4)
    before = chunk.psi.copy()
    small = HostChunk(np.zeros(1 << (n - 1)))
    zero = HostChunk(np.zeros(1 << n))
    for call in (lambda: krylov.ground_state(chunk, work[:3], None, obs, m=4),        # too few work chunks
                 lambda: krylov.ground_state(chunk, work, None, obs, m=1),            # m < 2
                 lambda: krylov.ground_state(zero, work, None, obs, m=4),             # a zero start vector
                 lambda: krylov.ground_state(chunk, [chunk] + work[:3], None, obs, m=4),
                 lambda: krylov.ground_state(chunk, work[:3] + [small], None, obs, m=4),
                 lambda: krylov.ground_state(chunk, work, [0, 1, 2, 2], obs, m=4),    # not a layout
                 lambda: krylov.ground_state(chunk, work, None, PauliSum({"X5": 1.0}), m=4),
                 lambda: krylov.lanczos(chunk, work, None, obs, 5),
                 lambda: krylov.lanczos(chunk, work, None, obs, 0),
                 lambda: krylov.lanczos(zero, work, None, obs, 4),
                 lambda: krylov.evolve(chunk, work, None, obs, 0.1, m=5),
                 lambda: krylov.evolve(chunk, work, None, obs, 0.1, m=4, steps=0),
                 lambda: krylov.evolve(chunk, work, None, obs, float("nan"), m=4),
                 lambda: krylov.evolve(zero, work, None, obs, 0.1, m=4)):
        with pytest.raises(ValueError):
            call()
    assert np.array_equal(chunk.psi, before) and not chunk.calls                      # refused before anything ran
