"""What one reads off a reduced density matrix, and the entanglement of a cut (host-only numpy on the result).

`DeviceChunk.reduced_density_matrix` (1 to 6 qubits, at most 64 x 64), `DeviceChunk.reduced_density_matrix_wide` (7 to
12 qubits, at most 4096 x 4096), `SingleGpuEngine.reduced_density_matrix` and `single_node.reduced_density_matrix`
return rho_A = Tr_rest |psi><psi| unnormalised (its trace is sum |amp|^2).  `normalised`, `purity`, `entropy` and
`fidelity_with_pure` accept that, of any size, and divide by the trace themselves.

`subsystem`, `schmidt_spectrum`, `entanglement_entropy` and `entropy_profile` take a state in a layout, `(chunk, l2p)`
(logical qubit q on index bit l2p[q]; None: the identity), and LOGICAL qubits; the state does not move.  On an engine or
a buffer `h` they are called as `density.<fn>(h.state, h.l2p, ...)`.  The matrix comes from the device, its eigenvalues
from `numpy.linalg.eigvalsh` on the host.
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


MAX_SUBSYSTEM = 12      # qubits of the widest matrix the device computes (reduced_density_matrix_wide)
_NARROW = 6             # ... of reduced_density_matrix


def _qubit_list(chunk, l2p, qubits, what: str):
    n = chunk.k if l2p is None else len(l2p)
    qs = [int(q) for q in qubits]
    if len(set(qs)) != len(qs):
        raise ValueError(f"{what}: repeated qubit in {qs}")
    if any(q < 0 or q >= n for q in qs):
        raise ValueError(f"{what}: qubits {qs} outside 0..{n - 1}")
    return n, qs


def subsystem(chunk, l2p, qubits) -> np.ndarray:
    """rho_A of 1 to 12 LOGICAL qubits, unnormalised, complex128 (2^r, 2^r), bit j of a row or column index = qubit
    qubits[j]: `chunk.reduced_density_matrix` for 1 to 6 qubits, `chunk.reduced_density_matrix_wide` for 7 to 12."""
    _, qs = _qubit_list(chunk, l2p, qubits, "subsystem")
    if not 1 <= len(qs) <= MAX_SUBSYSTEM:
        raise ValueError(f"subsystem: 1 to {MAX_SUBSYSTEM} qubits expected, got {len(qs)}")
    phys = qs if l2p is None else [int(l2p[q]) for q in qs]
    return chunk.reduced_density_matrix(phys) if len(qs) <= _NARROW else chunk.reduced_density_matrix_wide(phys)


def schmidt_spectrum(chunk, l2p, qubits) -> np.ndarray:
    """The eigenvalues of rho_A / Tr rho_A across the cut A = `qubits` | rest, descending, clipped at 0: the squared
    Schmidt coefficients.  The state on the chunk is pure, so both sides of the cut have the same nonzero spectrum and
    the SMALLER side is evaluated: when 2 |A| > n the complement, ascending.  The smaller side may have at most 12
    qubits."""
    n, qs = _qubit_list(chunk, l2p, qubits, "schmidt_spectrum")
    if not 1 <= len(qs) <= n - 1:
        raise ValueError(f"schmidt_spectrum: a cut of {n} qubits has 1 to {n - 1} of them on one side, got {len(qs)}")
    if min(len(qs), n - len(qs)) > MAX_SUBSYSTEM:
        raise ValueError(f"schmidt_spectrum: the cut {len(qs)} | {n - len(qs)} has more than {MAX_SUBSYSTEM} qubits on both sides")
    if 2 * len(qs) > n:
        inside = set(qs)
        qs = [q for q in range(n) if q not in inside]
    rho = normalised(subsystem(chunk, l2p, qs))
    lam = np.linalg.eigvalsh(rho)
    return np.clip(lam, 0.0, None)[::-1].copy()


def _entropy_of(lam: np.ndarray, base: float, alpha: float) -> float:
    lam = lam[lam > 0.0]
    if alpha == 1:
        return float(-np.sum(lam * np.log(lam)) / np.log(base))
    return float(np.log(np.sum(lam ** alpha)) / ((1.0 - alpha) * np.log(base)))


def entanglement_entropy(chunk, l2p, qubits, base: float = 2, alpha: float = 1) -> float:
    """Entanglement entropy across the cut `qubits` | rest from `schmidt_spectrum`: von Neumann -sum lam log lam for
    alpha = 1, otherwise the Renyi entropy log(sum lam^alpha) / (1 - alpha); in units of log(base)."""
    if alpha != 1 and (not alpha > 0 or not np.isfinite(alpha)):
        raise ValueError(f"entanglement_entropy: alpha = {alpha}: a positive finite number expected")
    return _entropy_of(schmidt_spectrum(chunk, l2p, qubits), base, alpha)


def entropy_profile(chunk, l2p, order=None, base: float = 2) -> np.ndarray:
    """Von Neumann entropies of the n - 1 cuts {order[0..m)} | rest, m = 1 .. n - 1, as an array (entry m - 1).  `order`
    is a permutation of the logical qubits (default 0 .. n - 1: the cuts of a chain).  NaN where both sides of the cut
    have more than 12 qubits."""
    n = chunk.k if l2p is None else len(l2p)
    order = list(range(n)) if order is None else [int(q) for q in order]
    if sorted(order) != list(range(n)):
        raise ValueError(f"entropy_profile: order must be a permutation of 0..{n - 1}, got {order}")
    out = np.full(max(n - 1, 0), np.nan)
    for m in range(1, n):
        if min(m, n - m) <= MAX_SUBSYSTEM:
            out[m - 1] = entanglement_entropy(chunk, l2p, order[:m], base)
    return out
