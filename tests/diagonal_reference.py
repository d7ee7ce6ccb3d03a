"""numpy reference of the diagonal Pauli sums D = sum_t c_t Z^{z_t} (qsim_apply_diagonal_phase, qsim_diagonal_moments):
E(i) = sum_t c_t (-1)^popcount(i & z_t) by the direct sum over the terms, no transform anywhere.

    energies(n, z, c)          -> E over the 2^n indices
    phase(psi, z, c, gamma)    -> exp(-i gamma D) psi
    moments(psi, z, c)         -> (sum |psi|^2, sum |psi|^2 E, sum |psi|^2 E^2), unnormalised
"""
import numpy as np


def _signs(idx: np.ndarray, masks: np.ndarray) -> np.ndarray:
    """(-1)^popcount(i & m) for every index i (rows) and mask m (columns), as float64."""
    par = np.bitwise_count(idx[:, None] & masks[None, :]) & np.uint8(1)
    return 1.0 - 2.0 * par.astype(np.float64)


def energies_naive(n: int, z, c) -> np.ndarray:
    """The definition, term by term in list order (small n: the check of `energies`)."""
    i = np.arange(1 << n, dtype=np.uint64)
    e = np.zeros(1 << n, dtype=np.float64)
    for zt, ct in zip(np.asarray(z, dtype=np.uint64).reshape(-1), np.asarray(c, dtype=np.float64).reshape(-1)):
        e += float(ct) * _signs(i, np.array([zt], dtype=np.uint64))[:, 0]
    return e


def energies(n: int, z, c) -> np.ndarray:
    """E(i) for i < 2^n by the direct sum over the terms.  The sign of a term factors over the index bits,
    (-1)^popcount(i & z) = s(i_hi, z_hi) s(i_lo, z_lo), so the sum over t of c_t s_hi s_lo is written as ONE matrix product
    (2^(n - h) x T) @ (T x 2^h): the same T products per index as the term loop, none left out and nothing transformed."""
    z = np.asarray(z, dtype=np.uint64).reshape(-1)
    c = np.asarray(c, dtype=np.float64).reshape(-1)
    if z.shape != c.shape:
        raise ValueError(f"{z.size} masks, {c.size} coefficients")
    if np.any(z >> np.uint64(n)):
        raise ValueError(f"a mask has a bit >= {n}")
    h = n // 2
    lo = np.arange(1 << h, dtype=np.uint64)
    hi = np.arange(1 << (n - h), dtype=np.uint64)
    if z.size == 0:
        return np.zeros(1 << n, dtype=np.float64)
    a = _signs(hi, z >> np.uint64(h)) * c[None, :]
    b = _signs(lo, z & np.uint64((1 << h) - 1))
    return (a @ b.T).reshape(-1)


def phase(psi: np.ndarray, z, c, gamma: float) -> np.ndarray:
    psi = np.asarray(psi, dtype=np.complex128)
    n = psi.size.bit_length() - 1
    return psi * np.exp(-1j * float(gamma) * energies(n, z, c))


def moments(psi: np.ndarray, z, c) -> tuple:
    psi = np.asarray(psi, dtype=np.complex128)
    n = psi.size.bit_length() - 1
    p = psi.real ** 2 + psi.imag ** 2
    e = energies(n, z, c)
    return float(np.sum(p)), float(np.sum(p * e)), float(np.sum(p * e * e))


class FakeChunk:
    """A host stand-in for `DeviceChunk` that applies the numpy references and records the calls it gets: the host
    bookkeeping of `diagonal` and of `evolution.apply_rotations(fuse_diagonal=True)` runs against it without a GPU."""

    def __init__(self, psi):
        self.psi = np.array(psi, dtype=np.complex128)
        self.k = self.psi.size.bit_length() - 1
        self.calls = []

    def apply_diagonal_phase(self, z_masks, coeffs, gamma):
        z, co = np.array(z_masks, dtype=np.uint64), np.array(coeffs, dtype=np.float64)
        self.calls.append(("diagonal", z, co, float(gamma)))
        self.psi = phase(self.psi, z, co, gamma)

    def diagonal_moments(self, z_masks, coeffs):
        self.calls.append(("moments", np.array(z_masks, dtype=np.uint64), np.array(coeffs, dtype=np.float64)))
        return moments(self.psi, z_masks, coeffs)

    def apply_pauli_rotations(self, x_masks, z_masks, thetas):
        from tests.rotation_reference import rotate_list
        x, z, th = np.array(x_masks, dtype=np.uint64), np.array(z_masks, dtype=np.uint64), np.array(thetas, dtype=np.float64)
        self.calls.append(("rotations", x, z, th))
        self.psi = rotate_list(self.psi, x, z, th)
        return 1 if x.size else 0
