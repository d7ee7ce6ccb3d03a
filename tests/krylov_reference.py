"""Host references for qsim_lincomb and quantum_simulations_amd.krylov: the linear combination with its dots and norm
in numpy, the dense matrix of a Pauli sum built string by string from tests/pauli_reference.apply_pauli, the two model
Hamiltonians of the Krylov tests, and a numpy stand-in chunk with the calls `krylov` makes (precedent: HostChunk in
tests/test_hamiltonian_cpu.py)."""
import numpy as np

from quantum_simulations_amd.observable import PauliSum
from tests.pauli_reference import apply_pauli
from tests.twostate_reference import apply_sum


def lincomb(dst, dst_coeff, srcs=(), coeffs=(), bras=(), want_norm2=False):
    """(new dst, dots, norm2 or None) of qsim_lincomb: a_d dst first (dst is not read for a_d == 0), then the sources in
    list order; the dots <bra|new dst> and the norm of the NEW dst."""
    dst_coeff = complex(dst_coeff)
    new = np.zeros(len(dst), dtype=np.complex128) if dst_coeff == 0 else dst_coeff * np.asarray(dst, dtype=np.complex128)
    for a, s in zip(coeffs, srcs):
        new = new + complex(a) * np.asarray(s, dtype=np.complex128)
    dots = np.array([np.vdot(b, new) for b in bras], dtype=np.complex128)
    return new, dots, (float(np.vdot(new, new).real) if want_norm2 else None)


def dense_matrix(obs: PauliSum, n: int) -> np.ndarray:
    """The 2^n x 2^n matrix of a Pauli sum over logical qubits (qubit q = bit q of the index).  A string has one entry
    per row, P[i, i ^ x]; apply_pauli on the all-ones vector reads it off: (P 1)_i = P[i, i ^ x]."""
    dim = 1 << n
    i = np.arange(dim)
    H = np.zeros((dim, dim), dtype=np.complex128)
    for c, x, z in zip(obs.coeffs, obs.x, obs.z):
        H[i, i ^ int(x)] += float(c) * apply_pauli(np.ones(dim, dtype=np.complex128), int(x), int(z))
    return H


class Spectrum:
    """The eigen-decomposition of a REAL symmetric Pauli sum, sector by sector: `key` (an integer per basis state that H
    conserves, e.g. the popcount for the Heisenberg chain; None: one sector) splits the matrix into independent blocks,
    so 12 qubits cost a few 924 x 924 problems instead of one 4096 x 4096."""

    def __init__(self, obs: PauliSum, n: int, key=None):
        H = dense_matrix(obs, n)
        assert not np.any(H.imag)
        key = np.zeros(1 << n, dtype=int) if key is None else np.asarray(key)
        self.sectors = []
        covered = 0.0
        for s in np.unique(key):
            idx = np.flatnonzero(key == s)
            block = H.real[np.ix_(idx, idx)]
            covered += float(np.sum(block * block))
            self.sectors.append((idx,) + tuple(np.linalg.eigh(block)))
        assert abs(covered - float(np.sum(H.real * H.real))) < 1e-9              # `key` is conserved: nothing outside the blocks
        self.e0 = min(lam[0] for _, lam, _ in self.sectors)

    def evolve(self, psi: np.ndarray, t) -> np.ndarray:
        """exp(-i t H) psi (t may be complex)."""
        out = np.zeros(psi.size, dtype=np.complex128)
        for idx, lam, U in self.sectors:
            out[idx] = U @ (np.exp(-1j * t * lam) * (U.T @ psi[idx]))
        return out


def popcount(n: int) -> np.ndarray:
    return np.array([bin(i).count("1") for i in range(1 << n)])


def ising_chain(n: int, h: float = 1.5) -> PauliSum:
    """Open transverse-field Ising chain -sum Z_q Z_{q+1} - h sum X_q."""
    terms = [(-1.0, {q: "Z", q + 1: "Z"}) for q in range(n - 1)] + [(-h, {q: "X"}) for q in range(n)]
    return PauliSum(terms, n_qubits=n)


def heisenberg_chain(n: int) -> PauliSum:
    """Open Heisenberg chain sum_q (X X + Y Y + Z Z)_{q, q+1}."""
    return PauliSum([(1.0, {q: p, q + 1: p}) for q in range(n - 1) for p in "XYZ"], n_qubits=n)


def zz_chain(n: int) -> PauliSum:
    """Diagonal: every basis state is an eigenstate."""
    return PauliSum([(-1.0 - 0.1 * q, {q: "Z", q + 1: "Z"}) for q in range(n - 1)], n_qubits=n)


def rand_state(n: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    psi = rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)
    return psi / np.linalg.norm(psi)


def to_physical_state(logical: np.ndarray, l2p) -> np.ndarray:
    """The array a chunk holds when its logical qubit q lives on index bit l2p[q]."""
    i = np.arange(logical.size)
    y = np.zeros_like(i)
    for q, p in enumerate(l2p):
        y |= ((i >> p) & 1) << q
    return logical[y]


class HostChunk:
    """The chunk calls `krylov` makes, on a numpy array of 2^k amplitudes (masks over PHYSICAL index bits)."""

    def __init__(self, psi):
        self.psi = np.array(psi, dtype=np.complex128)
        self.k = self.psi.size.bit_length() - 1
        self.calls = []

    def apply_pauli_sum(self, src, x, z, coeffs):
        assert src is not self
        self.calls.append(("sum", len(coeffs)))
        self.psi = apply_sum(src.psi, x, z, coeffs)
        return 1

    def lincomb(self, dst_coeff, srcs=(), coeffs=(), bras=(), want_norm2=False):
        srcs, bras = list(srcs), list(bras)
        assert len(srcs) <= 4 and len(bras) <= 4 and len(coeffs) == len(srcs)
        assert all(c is not self for c in srcs + bras)
        self.calls.append(("lincomb", len(srcs), len(bras), bool(want_norm2)))
        self.psi, dots, norm2 = lincomb(self.psi, dst_coeff, [s.psi for s in srcs], coeffs, [b.psi for b in bras], want_norm2)
        return dots, norm2

    def copy_from(self, other):
        self.psi = other.psi.copy()

    def norm2(self):
        return float(np.vdot(self.psi, self.psi).real)
