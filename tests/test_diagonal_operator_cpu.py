"""The host side of the diagonal Pauli sum as an operator, without a GPU: the reference gradient of
tests/diagonal_operator_reference against central differences, then `diagonal.qaoa_gradient`, `hamiltonian.apply(...,
fuse_diagonal=True)` and `krylov.lanczos(..., fuse_diagonal=True)` on its HostChunk (numpy references, calls recorded)."""
import numpy as np
import pytest

from quantum_simulations_amd import diagonal, hamiltonian, krylov
from quantum_simulations_amd.observable import PauliSum
from tests import diagonal_operator_reference as dref
from tests.krylov_reference import dense_matrix, heisenberg_chain, ising_chain, rand_state, to_physical_state


def _cost(n, seed):
    """All pairs and a few single Z, random weights, sum |c| = 1."""
    rng = np.random.default_rng(seed)
    terms = [(float(rng.standard_normal()), {a: "Z", b: "Z"}) for a in range(n) for b in range(a + 1, n)]
    terms += [(float(rng.standard_normal()), {q: "Z"}) for q in range(0, n, 2)] + [(0.3, {})]
    s = sum(abs(c) for c, _ in terms)
    return PauliSum([(c / s, ops) for c, ops in terms], n_qubits=n)


GAMMAS, BETAS = np.array([2.9, -3.4]), np.array([0.7, -0.45])


@pytest.mark.parametrize("n", [4, 5])
def test_reference_gradient_against_central_differences(n):
    cost = _cost(n, n)
    z, co = diagonal.diagonal_part(cost)
    psi = rand_state(n, 10 + n)
    energy, dg, db = dref.qaoa_gradient(psi, z, co, GAMMAS, BETAS)
    assert abs(energy - dref.qaoa_energy(psi, z, co, GAMMAS, BETAS)) < 1e-14
    h = 1e-5
    for l in range(GAMMAS.size):
        e = np.zeros(GAMMAS.size)
        e[l] = h
        num_g = (dref.qaoa_energy(psi, z, co, GAMMAS + e, BETAS) - dref.qaoa_energy(psi, z, co, GAMMAS - e, BETAS)) / (2 * h)
        num_b = (dref.qaoa_energy(psi, z, co, GAMMAS, BETAS + e) - dref.qaoa_energy(psi, z, co, GAMMAS, BETAS - e)) / (2 * h)
        print(f"n={n} layer {l}: dgamma {dg[l]:+.10f} (differences {num_g:+.10f}), dbeta {db[l]:+.10f} ({num_b:+.10f})")
        assert abs(dg[l] - num_g) < 1e-7 and abs(db[l] - num_b) < 1e-7
    assert float(np.max(np.abs(dg))) > 1e-3 and float(np.max(np.abs(db))) > 1e-3
    # against the dense matrix of the cost
    C = dense_matrix(cost, n)
    ket, bra = rand_state(n, 1), rand_state(n, 2)
    assert float(np.max(np.abs(dref.apply_sum(ket, z, co) - C @ ket))) < 1e-14
    ov, el = dref.matrix_element(ket, bra, z, co)
    assert abs(ov - np.vdot(bra, ket)) < 1e-15 and abs(el - np.vdot(bra, C @ ket)) < 1e-14


@pytest.mark.parametrize("l2p", [None, [3, 0, 4, 1, 2]])
def test_qaoa_gradient_on_the_host_chunk(l2p):
    n = 5
    cost = _cost(n, 7)
    z, co = diagonal.diagonal_part(cost)
    logical = rand_state(n, 8)
    physical = logical if l2p is None else to_physical_state(logical, l2p)
    chunk, work = dref.HostChunk(physical), dref.HostChunk(np.zeros(1 << n))
    energy, dg, db = diagonal.qaoa_gradient(chunk, work, l2p, cost, GAMMAS, BETAS)
    want_e, want_g, want_b = dref.qaoa_gradient(logical, z, co, GAMMAS, BETAS)
    assert abs(energy - want_e) < 1e-13
    assert float(np.max(np.abs(dg - want_g))) < 1e-13 and float(np.max(np.abs(db - want_b))) < 1e-13
    assert float(np.max(np.abs(chunk.psi - physical))) < 1e-13               # psi_0 again
    kinds = [c[0] for c in chunk.calls]
    assert kinds == ["diagonal", "rotations"] * 2 + ["moments"] + ["overlap", "rotations", "diagonal_overlap", "diagonal"] * 2
    assert [c[0] for c in work.calls] == ["diagonal_sum"] + ["rotations", "diagonal"] * 2
    assert work.calls[0][3] is False
    if l2p is not None:                                                      # the masks of every call are physical
        want_z = [sum(1 << l2p[q] for q in range(n) if (int(m) >> q) & 1) for m in z]
        assert work.calls[0][1].tolist() == want_z
        assert chunk.calls[5][1].tolist() == [1 << l2p[q] for q in range(n)]
    # matrix_element and apply_sum through the same layout
    other = dref.HostChunk(rand_state(n, 9))
    ov, el = diagonal.matrix_element(chunk, other, l2p, cost)
    unlay = (lambda v: v) if l2p is None else (lambda v: _to_logical(v, l2p))
    want = dref.matrix_element(unlay(chunk.psi), unlay(other.psi), z, co)
    assert abs(ov - want[0]) < 1e-14 and abs(el - want[1]) < 1e-14
    before = other.psi.copy()
    assert diagonal.apply_sum(other, chunk, l2p, cost, accumulate=True) == 1
    assert float(np.max(np.abs(unlay(other.psi) - unlay(before) - dref.apply_sum(unlay(chunk.psi), z, co)))) < 1e-14
    assert diagonal.apply_sum(other, other, l2p, cost) == 1                  # in place
    assert diagonal.apply_sum(other, chunk, l2p, PauliSum([], n_qubits=n)) == 0


def _to_logical(physical, l2p):
    from quantum_simulations_amd.circuit.staging import permute_state
    return permute_state(physical, l2p)


def test_apply_fuse_diagonal(monkeypatch):
    n = 6
    H = heisenberg_chain(n)                                                  # 5 ZZ bonds among 15 terms
    x, z = H.masks(None)
    n_diag = int(np.count_nonzero(x == 0))
    assert n_diag == n - 1
    src = dref.HostChunk(rand_state(n, 3))
    plain = dref.HostChunk(np.zeros(1 << n))
    assert hamiltonian.apply(plain, src, None, H) == 1
    assert [c[0] for c in plain.calls] == ["sum"] and plain.calls[0][3].size == len(H)
    # below the threshold (the default, a model of 30 qubits, is far above 5 terms): the per-term path
    assert hamiltonian.DIAGONAL_MIN_TERMS > n_diag
    low = dref.HostChunk(np.zeros(1 << n))
    hamiltonian.apply(low, src, None, H, fuse_diagonal=True)
    assert [c[0] for c in low.calls] == ["sum"] and low.calls[0][3].size == len(H)
    monkeypatch.setattr(hamiltonian, "DIAGONAL_MIN_TERMS", n_diag + 1)
    hamiltonian.apply(low, src, None, H, fuse_diagonal=True)
    assert [c[0] for c in low.calls] == ["sum", "sum"]
    # at the threshold: the rest writes, then exactly the Z-only terms accumulate
    monkeypatch.setattr(hamiltonian, "DIAGONAL_MIN_TERMS", n_diag)
    for l2p in (None, [5, 2, 0, 3, 1, 4]):
        px, pz = H.masks(l2p)
        s = dref.HostChunk(src.psi if l2p is None else to_physical_state(src.psi, l2p))
        unfused, fused = dref.HostChunk(np.ones(1 << n)), dref.HostChunk(np.ones(1 << n))
        hamiltonian.apply(unfused, s, l2p, H)
        assert hamiltonian.apply(fused, s, l2p, H, fuse_diagonal=True) == 2
        assert [c[0] for c in fused.calls] == ["sum", "diagonal_sum"]
        assert fused.calls[0][1].tolist() == px[px != 0].tolist() and fused.calls[0][3].tolist() == H.coeffs[px != 0].tolist()
        assert fused.calls[1][1].tolist() == pz[px == 0].tolist() and fused.calls[1][2].tolist() == H.coeffs[px == 0].tolist()
        assert fused.calls[1][3] is True
        assert float(np.max(np.abs(fused.psi - unfused.psi))) < 1e-13
    # no rest: the diagonal pass writes
    D = PauliSum([(0.5 + 0.1 * q, {q: "Z", q + 1: "Z"}) for q in range(n - 1)] + [(0.25, {})], n_qubits=n)
    only = dref.HostChunk(np.ones(1 << n))
    assert hamiltonian.apply(only, src, None, D, fuse_diagonal=True) == 1
    assert [c[0] for c in only.calls] == ["diagonal_sum"] and only.calls[0][3] is False and only.calls[0][1].size == n
    assert float(np.max(np.abs(only.psi - dense_matrix(D, n) @ src.psi))) < 1e-13
    # variance hands the flag on
    T = ising_chain(n)
    a, b = dref.HostChunk(np.zeros(1 << n)), dref.HostChunk(np.zeros(1 << n))
    v0 = hamiltonian.variance(src, a, None, T)
    v1 = hamiltonian.variance(src, b, None, T, fuse_diagonal=True)
    assert [c[0] for c in b.calls] == ["sum", "diagonal_sum"] and abs(v0 - v1) < 1e-13


def test_lanczos_fuse_diagonal(monkeypatch):
    n, m = 6, 5
    monkeypatch.setattr(hamiltonian, "DIAGONAL_MIN_TERMS", 2)
    for H in (ising_chain(n), heisenberg_chain(n)):
        runs = []
        for fuse in (False, True):
            chunk = dref.HostChunk(rand_state(n, 4))
            work = [dref.HostChunk(np.zeros(1 << n)) for _ in range(m)]
            alphas, betas, k = krylov.lanczos(chunk, work, None, H, m, fuse_diagonal=fuse)
            assert k == m
            applied = [c[0] for w in work for c in w.calls if c[0] in ("sum", "diagonal_sum")]
            assert applied == (["sum", "diagonal_sum"] * m if fuse else ["sum"] * m)
            runs.append((alphas, betas))
        assert float(np.max(np.abs(runs[0][0] - runs[1][0]))) < 1e-12 and float(np.max(np.abs(runs[0][1] - runs[1][1]))) < 1e-12
    # ground_state and evolve take the flag and make the same calls
    H = ising_chain(n)
    chunk = dref.HostChunk(rand_state(n, 5))
    work = [dref.HostChunk(np.zeros(1 << n)) for _ in range(m)]
    energy, residual, restarts, _ = krylov.ground_state(chunk, work, None, H, m, tol=1e-9, max_restarts=60, fuse_diagonal=True)
    assert residual <= 1e-9 and abs(energy - float(np.linalg.eigvalsh(dense_matrix(H, n).real)[0])) < 1e-9
    assert any(c[0] == "diagonal_sum" for c in work[0].calls)                # the residual's H application too
    before = chunk.psi.copy()
    krylov.evolve(chunk, work, None, H, 0.1, m, fuse_diagonal=True)
    lam, U = np.linalg.eigh(dense_matrix(H, n))
    assert float(np.max(np.abs(chunk.psi - (U * np.exp(-0.1j * lam)) @ (U.conj().T @ before)))) < 1e-9


def test_argument_errors():
    n = 4
    cost = _cost(n, 1)
    chunk, work = dref.HostChunk(rand_state(n, 1)), dref.HostChunk(np.zeros(1 << n))
    small = dref.HostChunk(np.zeros(1 << (n - 1)))
    with pytest.raises(ValueError, match="gammas"):
        diagonal.qaoa_gradient(chunk, work, None, cost, [0.1, 0.2], [0.3])
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="finite"):
            diagonal.qaoa_gradient(chunk, work, None, cost, [bad], [0.3])
        with pytest.raises(ValueError, match="finite"):
            diagonal.qaoa_gradient(chunk, work, None, cost, [0.1], [bad])
    with pytest.raises(ValueError, match="different"):
        diagonal.qaoa_gradient(chunk, chunk, None, cost, [0.1], [0.3])
    with pytest.raises(ValueError, match="index bits"):
        diagonal.qaoa_gradient(chunk, small, None, cost, [0.1], [0.3])
    with pytest.raises(ValueError, match="not diagonal"):
        diagonal.qaoa_gradient(chunk, work, None, {"X0": 1.0}, [0.1], [0.3])
    with pytest.raises(ValueError, match="not diagonal"):
        diagonal.apply_sum(work, chunk, None, {"Z0 Y1": 1.0})
    with pytest.raises(ValueError, match="not diagonal"):
        diagonal.matrix_element(chunk, work, None, {"X2": 1.0})
    with pytest.raises(ValueError, match="index bits"):
        diagonal.apply_sum(small, chunk, None, cost)
    with pytest.raises(ValueError, match="index bits"):
        diagonal.matrix_element(chunk, small, None, cost)
    with pytest.raises(ValueError, match="different"):
        hamiltonian.apply(chunk, chunk, None, cost, fuse_diagonal=True)
    assert chunk.calls == [] and work.calls == []                            # refused before any chunk call
    # no layers: the energy of the state itself, no derivative
    energy, dg, db = diagonal.qaoa_gradient(chunk, work, None, cost, [], [])
    z, co = diagonal.diagonal_part(cost)
    assert abs(energy - dref.matrix_element(chunk.psi, chunk.psi, z, co)[1].real) < 1e-14 and dg.size == 0 and db.size == 0
