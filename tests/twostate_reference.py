"""Host references (numpy) of the two-state calls: a Pauli sum applied as an operator, matrix elements between two
states, and the gradient of <psi(theta)|H|psi(theta)> over a rotation list.  Everything is built on
pauli_reference.apply_pauli (axis flips and sign vectors, no index arithmetic), so what it shares with the device kernels
is the definition alone.  Pinned against explicit Kronecker matrices and central differences in
tests/test_hamiltonian_cpu.py.

`gradient_forward` is deliberately NOT the adjoint recursion that quantum_simulations_amd.hamiltonian runs: parameter j
gets d_j psi = R_{n-1} .. R_{j+1} (-i P_j) R_j .. R_0 psi_0 by running the rest of the list forward from the insertion,
and dE/dtheta_j = 2 Re <psi|H|d_j psi>: O(n^2) rotations."""
import numpy as np

from tests.pauli_reference import apply_pauli
from tests.rotation_reference import rotate


def apply_sum(psi: np.ndarray, xs, zs, coeffs) -> np.ndarray:
    """sum_t coeffs[t] P_t |psi>."""
    psi = np.asarray(psi, dtype=np.complex128)
    out = np.zeros_like(psi)
    for x, z, c in zip(xs, zs, coeffs):
        out += float(c) * apply_pauli(psi, int(x), int(z))
    return out


def matrix_elements(bra: np.ndarray, ket: np.ndarray, xs, zs) -> np.ndarray:
    """<bra|P_t|ket> of every string, complex."""
    bra = np.asarray(bra, dtype=np.complex128)
    return np.array([np.vdot(bra, apply_pauli(ket, int(x), int(z))) for x, z in zip(xs, zs)], dtype=np.complex128)


def energy(psi0: np.ndarray, rot_x, rot_z, thetas, hx, hz, coeffs) -> float:
    """<psi|H|psi> after the rotation list (first entry first) is applied to psi0."""
    psi = np.asarray(psi0, dtype=np.complex128)
    for x, z, th in zip(rot_x, rot_z, thetas):
        psi = rotate(psi, int(x), int(z), float(th))
    return float(np.vdot(psi, apply_sum(psi, hx, hz, coeffs)).real)


def gradient_forward(psi0: np.ndarray, rot_x, rot_z, thetas, hx, hz, coeffs) -> tuple:
    """(E, dE/dtheta) with every list entry its own parameter; R = exp(-i theta P), no factor 1/2."""
    rot = [(int(x), int(z), float(th)) for x, z, th in zip(rot_x, rot_z, thetas)]
    prefix = [np.asarray(psi0, dtype=np.complex128)]           # prefix[j] = R_{j-1} .. R_0 psi0
    for x, z, th in rot:
        prefix.append(rotate(prefix[-1], x, z, th))
    psi = prefix[-1]
    hpsi = apply_sum(psi, hx, hz, coeffs)
    grad = np.zeros(len(rot), dtype=np.float64)
    for j, (x, z, _) in enumerate(rot):
        d = -1j * apply_pauli(prefix[j + 1], x, z)
        for xx, zz, th in rot[j + 1:]:
            d = rotate(d, xx, zz, th)
        grad[j] = 2.0 * np.vdot(hpsi, d).real
    return float(np.vdot(psi, hpsi).real), grad
