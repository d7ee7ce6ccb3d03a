"""What one reads off a reduced density matrix (host-only numpy, matrices of at most 64 x 64).

`DeviceChunk.reduced_density_matrix`, `SingleGpuEngine.reduced_density_matrix` and `single_node.reduced_density_matrix`
return rho_A = Tr_rest |psi><psi| unnormalised (its trace is sum |amp|^2).  Every function here accepts that and divides
by the trace itself.
"""
from __future__ import annotations

import numpy as np


def _square(rho) -> np.ndarray:
    rho = np.asarray(rho, dtype=np.complex128)
    if rho.ndim != 2 or rho.shape[0] != rho.shape[1] or rho.shape[0] == 0:
        raise ValueError(f"a square matrix expected, got shape {rho.shape}")
    return rho


def normalised(rho) -> np.ndarray:
    """rho / Tr rho."""
    rho = _square(rho)
    tr = float(np.trace(rho).real)
    if not tr > 0.0 or not np.isfinite(tr):
        raise ValueError(f"the trace is {tr}: a positive finite number expected")
    return rho / tr


def purity(rho) -> float:
    """Tr rho^2 / (Tr rho)^2: 1 for a pure state, 1 / dim for the maximally mixed one."""
    rho = normalised(rho)
    return float(np.sum(rho * rho.T).real)          # Tr rho rho = sum_ab rho_ab rho_ba


def entropy(rho, base: float = 2) -> float:
    """Von Neumann entropy -Tr rho log rho of rho / Tr rho, from the eigenvalues of the Hermitian part (eigvalsh).
    Eigenvalues below 0 (rounding) count as 0, and 0 log 0 = 0."""
    rho = normalised(rho)
    lam = np.linalg.eigvalsh((rho + rho.conj().T) / 2)
    lam = np.clip(lam, 0.0, None)
    lam = lam[lam > 0.0]
    return float(-np.sum(lam * np.log(lam)) / np.log(base))


def fidelity_with_pure(rho, phi) -> float:
    """<phi|rho|phi> / (Tr rho <phi|phi>): the fidelity of the subsystem's state with the pure state phi (entry a of
    phi <-> row a of rho)."""
    rho = normalised(rho)
    phi = np.asarray(phi, dtype=np.complex128).reshape(-1)
    if phi.size != rho.shape[0]:
        raise ValueError(f"phi has {phi.size} entries, rho is {rho.shape[0]} x {rho.shape[0]}")
    n2 = float(np.vdot(phi, phi).real)
    if not n2 > 0.0:
        raise ValueError("phi is the zero vector")
    return float(np.vdot(phi, rho @ phi).real / n2)
