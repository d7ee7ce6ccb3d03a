"""The host side of the diagonal Pauli sums without a GPU: `diagonal.diagonal_part` / `split` / the layout, the cut of a
rotation list for `fuse_diagonal`, and `diagonal.qaoa` against dense matrices, all on tests/diagonal_reference.FakeChunk
(a chunk that applies the numpy references and records its calls).  The reference itself is checked against the
term-by-term definition first."""
import numpy as np
import pytest

from quantum_simulations_amd import diagonal, evolution
from quantum_simulations_amd.circuit.staging import permute_state
from quantum_simulations_amd.observable import PauliSum
from tests import diagonal_reference as ref
from tests.rotation_reference import rotate_list


def _rand_state(n, seed):
    rng = np.random.default_rng(seed)
    psi = rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)
    return psi / np.linalg.norm(psi)


def _dense(obs: PauliSum) -> np.ndarray:
    """The 2^n x 2^n matrix of a Pauli sum (qubit q = bit q of the index)."""
    mats = {"I": np.eye(2), "X": np.array([[0, 1], [1, 0]]), "Y": np.array([[0, -1j], [1j, 0]]), "Z": np.diag([1.0, -1.0])}
    n = obs.n_qubits
    H = np.zeros((1 << n, 1 << n), dtype=np.complex128)
    for x, z, c in zip(obs.x, obs.z, obs.coeffs):
        M = np.eye(1, dtype=np.complex128)
        for q in range(n):
            bx, bz = (x >> q) & 1, (z >> q) & 1
            M = np.kron(mats["Y" if bx and bz else "X" if bx else "Z" if bz else "I"], M)
        H += c * M
    return H


def _expm_hermitian(H: np.ndarray, t: float) -> np.ndarray:
    w, v = np.linalg.eigh(H)
    return (v * np.exp(-1j * t * w)) @ v.conj().T


def test_reference_is_the_direct_sum():
    rng = np.random.default_rng(1)
    for n in (1, 2, 5, 9):
        z = rng.integers(0, 1 << n, size=37, dtype=np.uint64)
        c = rng.standard_normal(37)
        want = ref.energies_naive(n, z, c)
        assert float(np.max(np.abs(ref.energies(n, z, c) - want))) < 1e-13 * float(np.sum(np.abs(c)))
        # against the matrix of the Pauli sum
        obs = PauliSum([(float(ct), {q: "Z" for q in range(n) if (int(zt) >> q) & 1}) for zt, ct in zip(z, c)], n_qubits=n)
        assert float(np.max(np.abs(np.diag(_dense(obs)).real - want))) < 1e-12
    assert ref.energies(3, [], []).tolist() == [0.0] * 8
    psi = _rand_state(5, 2)
    z, c = np.array([0b101, 0, 0b10000], dtype=np.uint64), np.array([0.5, -2.0, 1.25])
    e = ref.energies_naive(5, z, c)
    assert np.allclose(ref.phase(psi, z, c, 0.3), psi * np.exp(-0.3j * e), atol=1e-15)
    p = np.abs(psi) ** 2
    assert np.allclose(ref.moments(psi, z, c), (p.sum(), (p * e).sum(), (p * e * e).sum()), atol=1e-14)


def test_diagonal_part_merges_and_rejects():
    obs = PauliSum([(0.5, {0: "Z", 3: "Z"}), (-1.0, {}), (0.25, {3: "Z", 0: "Z"}), (2.0, {1: "Z"})], n_qubits=5)
    z, c = diagonal.diagonal_part(obs)
    assert z.dtype == np.uint64 and c.dtype == np.float64
    assert z.tolist() == [0b1001, 0, 0b10] and c.tolist() == [0.75, -1.0, 2.0]
    # a sum that reaches diagonal_part with a repeated mask (built by hand: the constructor merges on its own)
    obs.x, obs.z, obs.coeffs = [0, 0, 0], [4, 1, 4], np.array([1.0, 2.0, 0.5])
    z, c = diagonal.diagonal_part(obs)
    assert z.tolist() == [4, 1] and c.tolist() == [1.5, 2.0]
    for bad in ({"X0": 1.0}, {"Z0 Y2": 1.0, "Z1": 2.0}, [(1.0, {0: "Z"}), (0.5, {1: "X", 0: "Z"})]):
        with pytest.raises(ValueError, match="not diagonal"):
            diagonal.diagonal_part(PauliSum(bad, n_qubits=3))
    z, c = diagonal.diagonal_part(PauliSum([], n_qubits=3))
    assert z.size == 0 and c.size == 0


def test_split():
    obs = PauliSum({"Z0 Z1": 1.0, "X0": -0.5, "I": 0.3, "Y1 Z2": 0.7, "Z2": 2.0}, n_qubits=3)
    diag, rest = diagonal.split(obs)
    assert diag.n_qubits == rest.n_qubits == 3
    assert diag.labels() == ["Z0 Z1", "I", "Z2"] and diag.coeffs.tolist() == [1.0, 0.3, 2.0]
    assert rest.labels() == ["X0", "Y1 Z2"] and rest.coeffs.tolist() == [-0.5, 0.7]
    assert np.allclose(_dense(diag) + _dense(rest), _dense(obs))
    assert len(diagonal.split(PauliSum({"X0": 1.0}, n_qubits=2))[0]) == 0


def test_phase_and_moments_through_a_shuffled_layout():
    n = 6
    l2p = [int(p) for p in np.random.default_rng(3).permutation(n)]
    obs = PauliSum({"Z0 Z5": 0.8, "Z2": -1.1, "I": 0.4, "Z1 Z3 Z4": 0.6}, n_qubits=n)
    logical = _rand_state(n, 4)
    # the chunk holds the state in the layout: permute_state(physical, l2p) is the logical vector
    idx = np.arange(1 << n)
    phys_of = np.zeros(1 << n, dtype=np.int64)
    for q, p in enumerate(l2p):
        phys_of |= ((idx >> q) & 1) << p
    physical = np.empty_like(logical)
    physical[phys_of] = logical
    assert np.array_equal(permute_state(physical, l2p), logical)
    chunk = ref.FakeChunk(physical)
    assert diagonal.apply_phase(chunk, l2p, obs, 0.37) == 1
    kind, z, co, gamma = chunk.calls[0]
    assert kind == "diagonal" and gamma == 0.37
    assert z.tolist() == [(1 << l2p[0]) | (1 << l2p[5]), 1 << l2p[2], 0, (1 << l2p[1]) | (1 << l2p[3]) | (1 << l2p[4])]
    want = _expm_hermitian(_dense(obs), 0.37) @ logical
    assert float(np.max(np.abs(permute_state(chunk.psi, l2p) - want))) < 1e-13
    mean, var = diagonal.moments(chunk, l2p, obs)
    H = _dense(obs)
    m1 = float(np.real(np.vdot(want, H @ want)))
    m2 = float(np.real(np.vdot(want, H @ (H @ want))))
    assert abs(mean - m1) < 1e-13 and abs(var - (m2 - m1 * m1)) < 1e-12
    assert diagonal.apply_phase(chunk, l2p, PauliSum([], n_qubits=n), 1.0) == 0
    with pytest.raises(ValueError):
        diagonal.apply_phase(chunk, l2p, obs, float("nan"))
    with pytest.raises(ValueError, match="not diagonal"):
        diagonal.apply_phase(chunk, l2p, {"X0": 1.0}, 0.1)


def test_diagonal_runs():
    Z, X = 0, 1
    cut = lambda xs, m: evolution.diagonal_runs(np.array(xs, dtype=np.uint64), m)
    assert cut([], 2) == []
    assert cut([X, X], 2) == [(0, 2, False)]
    assert cut([Z, Z, Z], 2) == [(0, 3, True)]
    assert cut([Z, Z, Z], 4) == [(0, 3, False)]
    assert cut([X, Z, Z, X, Z, X, Z, Z, Z], 2) == [(0, 1, False), (1, 3, True), (3, 6, False), (6, 9, True)]
    assert cut([X, Z, Z, X, Z, X, Z, Z, Z], 3) == [(0, 6, False), (6, 9, True)]
    assert cut([Z, X], 1) == [(0, 1, True), (1, 2, False)]
    assert evolution.DIAGONAL_MIN_RUN >= 1


def test_fuse_diagonal_sends_runs_to_the_diagonal_pass_in_order(monkeypatch):
    n = 5
    monkeypatch.setattr(evolution, "DIAGONAL_MIN_RUN", 3)
    rot = [("X0", 0.3), ("Z0 Z1", 0.2), ("Z2", -0.4), ("Z1 Z4", 0.9), ("Y3 Z0", 0.5), ("Z0", 0.7), ("Z3", -0.2), ("X1 X2", 0.1),
           ("Z0 Z1", 0.6), ("I", 0.8), ("Z4", -0.3)]
    x, z, th = evolution.as_rotation_arrays(rot)
    psi = _rand_state(n, 5)
    plain, fused = ref.FakeChunk(psi), ref.FakeChunk(psi)
    evolution.apply_rotations(plain, None, rot)
    assert [c[0] for c in plain.calls] == ["rotations"] and plain.calls[0][1].tolist() == x.tolist()
    passes = evolution.apply_rotations(fused, None, rot, fuse_diagonal=True)
    # [X0] | Z-run of 3 | [Y3Z0, Z0, Z3, X1X2] (a run of 2: stays a rotation) | Z-run of 3 (the identity among them)
    assert [c[0] for c in fused.calls] == ["rotations", "diagonal", "rotations", "diagonal"] and passes == 4
    assert fused.calls[0][1].tolist() == x[:1].tolist() and fused.calls[0][3].tolist() == th[:1].tolist()
    assert fused.calls[1][1].tolist() == z[1:4].tolist() and fused.calls[1][2].tolist() == th[1:4].tolist() and fused.calls[1][3] == 1.0
    assert fused.calls[2][1].tolist() == x[4:8].tolist() and fused.calls[2][2].tolist() == z[4:8].tolist()
    assert fused.calls[3][1].tolist() == z[8:].tolist() and fused.calls[3][2].tolist() == th[8:].tolist()
    want = rotate_list(psi, x, z, th)
    assert float(np.max(np.abs(plain.psi - want))) == 0.0
    assert float(np.max(np.abs(fused.psi - want))) < 1e-14
    # through a layout the masks of both kinds of call are physical
    l2p = [3, 0, 4, 1, 2]
    laid = ref.FakeChunk(psi)
    evolution.apply_rotations(laid, l2p, rot, fuse_diagonal=True)
    assert laid.calls[1][1].tolist() == [(1 << 3) | 1, 1 << 4, 1 | (1 << 2)]
    # evolve hands the flag on: the transverse-field Ising chain, the ZZ bonds first
    H = PauliSum([(1.0, {q: "Z", q + 1: "Z"}) for q in range(n - 1)] + [(0.7, {q: "X"}) for q in range(n)], n_qubits=n)
    ev = ref.FakeChunk(psi)
    assert evolution.evolve(ev, None, H, 0.2, steps=2, fuse_diagonal=True) == 4
    assert [c[0] for c in ev.calls] == ["diagonal", "rotations"] * 2
    assert float(np.max(np.abs(ev.psi - rotate_list(psi, *evolution.trotter_rotations(H, 0.2, 2))))) < 1e-14


def test_qaoa_against_dense_matrices():
    n = 4
    cost = PauliSum([(0.5, {a: "Z", b: "Z"}) for a, b in ((0, 1), (1, 2), (2, 3), (3, 0), (0, 2))] + [(-0.3, {1: "Z"}), (0.2, {})], n_qubits=n)
    mixer = PauliSum([(1.0, {q: "X"}) for q in range(n)], n_qubits=n)
    gammas, betas = [0.4, -0.9, 1.3], [0.7, 0.2, -0.5]
    plus = np.full(1 << n, 0.25, dtype=np.complex128)
    want = plus.copy()
    for g, b in zip(gammas, betas):
        want = _expm_hermitian(_dense(mixer), b) @ (_expm_hermitian(_dense(cost), g) @ want)
    for l2p in (None, [2, 0, 3, 1]):
        chunk = ref.FakeChunk(plus)                     # |+>^n is the same vector in every layout
        passes = diagonal.qaoa(chunk, l2p, cost, gammas, betas)
        assert passes == 6 and [c[0] for c in chunk.calls] == ["diagonal", "rotations"] * 3
        assert [c[3] for c in chunk.calls[0::2]] == gammas
        assert all(c[3].tolist() == [b] * n for c, b in zip(chunk.calls[1::2], betas))
        got = chunk.psi if l2p is None else permute_state(chunk.psi, l2p)
        assert float(np.max(np.abs(got - want))) < 1e-13
    # the mixer is RX(2 beta): no factor 1/2
    rx = lambda phi: np.array([[np.cos(phi / 2), -1j * np.sin(phi / 2)], [-1j * np.sin(phi / 2), np.cos(phi / 2)]])
    one = ref.FakeChunk(np.array([1.0, 0.0], dtype=np.complex128))
    diagonal.qaoa(one, None, PauliSum([], n_qubits=1), [0.0], [0.35])
    assert np.allclose(one.psi, rx(0.7)[:, 0], atol=1e-15)
    with pytest.raises(ValueError):
        diagonal.qaoa(ref.FakeChunk(plus), None, cost, [0.1, 0.2], [0.3])
