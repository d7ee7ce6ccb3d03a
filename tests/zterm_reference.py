"""numpy restatement of qsim_expectation_z_terms: the direct sum  out[t] = sum_i |psi_i|^2 (-1)^popcount(i & z_t),
unnormalised, in list order -- no transform, no tiles, nothing shared with the device code.  `HostZChunk` is the
stand-in chunk of the tests without a GPU: it answers the readout calls from these sums and records what it was asked."""
import numpy as np

from quantum_simulations_amd.observable import as_pauli_sum, pauli_terms_np


def parity(v: np.ndarray) -> np.ndarray:
    """popcount(v) & 1 of a uint64 array."""
    v = v.copy()
    for s in (32, 16, 8, 4, 2, 1):
        v ^= v >> np.uint64(s)
    return v & np.uint64(1)


def z_term_values(psi, z_masks) -> np.ndarray:
    """out[t] = sum_i |psi_i|^2 (-1)^popcount(i & z_masks[t]) (float64; numpy's pairwise sum of the signed weights)."""
    psi = np.asarray(psi, dtype=np.complex128).reshape(-1)
    p = psi.real * psi.real + psi.imag * psi.imag
    i = np.arange(p.size, dtype=np.uint64)
    out = np.empty(len(z_masks), dtype=np.float64)
    for t, z in enumerate(np.asarray(z_masks, dtype=np.uint64).reshape(-1)):
        out[t] = float(np.sum(np.where(parity(i & z) == 1, -p, p)))
    return out


def all_z_values(psi) -> np.ndarray:
    """Every Z string at once, entry z = sum_i |psi_i|^2 (-1)^popcount(i & z): a plain fast Walsh-Hadamard transform,
    for the stand-in library of the test with more than 16384 terms (checked against `z_term_values` there)."""
    psi = np.asarray(psi, dtype=np.complex128).reshape(-1)
    v = psi.real * psi.real + psi.imag * psi.imag
    h = 1
    while h < v.size:
        v = v.reshape(-1, 2, h)
        v = np.stack([v[:, 0, :] + v[:, 1, :], v[:, 0, :] - v[:, 1, :]], axis=1).reshape(-1)
        h *= 2
    return v


def correlations_np(psi, qubits, connected: bool):
    """(z, zz) of the normalised state over logical qubits `qubits` of psi (qubit q = index bit q)."""
    psi = np.asarray(psi, dtype=np.complex128).reshape(-1)
    p = np.abs(psi) ** 2
    p = p / p.sum()
    i = np.arange(p.size)
    s = np.array([1.0 - 2.0 * ((i >> q) & 1) for q in qubits])
    z = s @ p
    zz = (s * p) @ s.T
    return z, zz - np.outer(z, z) if connected else zz


class HostZChunk:
    """2^k amplitudes on the host with the readout calls of a `DeviceChunk` that the per-term paths use; `calls` holds
    (name, number of terms) of every call in order, `z_masks` the masks of the `expectation_z_terms` calls."""

    def __init__(self, psi):
        self.psi = np.asarray(psi, dtype=np.complex128).reshape(-1)
        self.k = self.psi.size.bit_length() - 1
        self.calls, self.z_masks = [], []

    def expectation_z_terms(self, z_masks):
        z = np.asarray(z_masks, dtype=np.uint64).reshape(-1)
        self.calls.append(("expectation_z_terms", int(z.size)))
        self.z_masks.append(z.copy())
        return z_term_values(self.psi, z)

    def expectation_pauli(self, x_masks, z_masks):
        self.calls.append(("expectation_pauli", len(x_masks)))
        return pauli_terms_np(self.psi, x_masks, z_masks)

    def expectation(self, obs, l2p=None):
        self.calls.append(("expectation", None))
        obs = as_pauli_sum(obs, self.k if l2p is None else len(l2p))
        return obs.value(pauli_terms_np(self.psi, *obs.masks(l2p)))
