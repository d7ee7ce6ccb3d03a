"""A Pauli sum H = sum_t c_t P_t as an OPERATOR on device states: H|psi> into a second chunk, matrix elements between
two chunks, the energy variance and adjoint-method gradients (qsim_apply_pauli_sum, qsim_overlap_pauli).

    apply(dst, src, l2p, obs, fuse_diagonal)                -> passes;  dst := H src, out of place
    plan(n_qubits, l2p, obs, fuse_diagonal)                 -> the masks of `apply` for a fixed H, made once
    apply_planned(dst, src, plan)                           -> passes;  what `apply` does with a plan
    matrix_elements(ket, bra, l2p, obs)                     -> complex array, <bra|P_t|ket> per term (no coefficients)
    variance(chunk, work, l2p, obs, fuse_diagonal)          -> norm2(H psi) - <H>^2, unnormalised
    adjoint_gradient(chunk, work, l2p, rotations, obs)      -> (energy, grad) of <psi(theta)|H|psi(theta)>

Everything here is host bookkeeping on small arrays: the chunks' logical qubit q lives on index bit l2p[q] (None:
identity) and the layout goes into the masks, as in `readout` and `evolution`; the amplitudes are touched by the device
only.  Both chunks of a call are of the same size, on the same device and in the same layout.

Gradient convention: NO factor 1/2, as everywhere in `evolution`.  A rotation is R(theta) = exp(-i theta P), so
d/dtheta R = -i P R, and the derivative returned is with respect to that theta (the derivative with respect to the
angle phi of a gate RZ(phi) = R(phi / 2) is half of it).
"""
from __future__ import annotations

import numpy as np

from quantum_simulations_amd import evolution
from quantum_simulations_amd.observable import as_pauli_sum

# Z-only terms from which `apply(fuse_diagonal=True)` sends them through one diagonal pass that accumulates (48 B per
# amplitude) instead of leaving them in the per-term passes.  MEASURED (profiles/r24_diagonal_operator_probe.json,
# `crossover`): inside a mixed sum a Z-only term costs the per-term passes about 0.40 ms at 30 qubits and 0.10 ms at 28,
# the extra pass 9.5 / 2.4 ms; on the Heisenberg and on the Ising chain, at both sizes, fusing loses up to 20 terms (by 2
# to 3 % at 20) and wins from 24 on: by 0.1 to 2 % at 24, which is the break-even, by 3 to 6 % at 28, by 31 to 39 % at 64.
DIAGONAL_MIN_TERMS = 24


class Plan:
    """The arrays of one H for `apply_planned`, over PHYSICAL index bits: (x, z, coeffs) of the terms that go through
    `apply_pauli_sum` and, when the Z-only terms take the diagonal pass, (diag_z, diag_coeffs), else None."""

    def __init__(self, x, z, coeffs, diag_z=None, diag_coeffs=None):
        self.x, self.z, self.coeffs, self.diag_z, self.diag_coeffs = x, z, coeffs, diag_z, diag_coeffs


def plan(n_qubits: int, l2p, obs, fuse_diagonal: bool = False) -> Plan:
    """The masks of a Pauli sum over LOGICAL qubits through the layout.  With `fuse_diagonal` the Z-only terms (the
    identity among them: what `diagonal.split` calls the diagonal part) are set apart for one diagonal pass when there
    are at least DIAGONAL_MIN_TERMS of them; fewer stay with the rest."""
    obs = as_pauli_sum(obs, n_qubits)
    x, z = obs.masks(l2p)
    co = np.asarray(obs.coeffs, dtype=np.float64)
    zonly = x == 0
    if not fuse_diagonal or int(np.count_nonzero(zonly)) < max(int(DIAGONAL_MIN_TERMS), 1):
        return Plan(x, z, co)
    return Plan(x[~zonly], z[~zonly], co[~zonly], z[zonly], co[zonly])


def apply_planned(dst, src, p: Plan) -> int:
    """dst := H src for the H of a `plan`.  Without a diagonal part: `apply_pauli_sum`.  With one: the rest through
    `apply_pauli_sum`, which writes, then the diagonal pass accumulates; with no rest the diagonal pass writes.  Returns
    the HBM passes made."""
    evolution.check_pair(dst, src, "apply")
    if p.diag_z is None:
        return dst.apply_pauli_sum(src, p.x, p.z, p.coeffs)
    passes = dst.apply_pauli_sum(src, p.x, p.z, p.coeffs) if p.x.size else 0
    dst.apply_diagonal_sum(src, p.diag_z, p.diag_coeffs, bool(p.x.size))
    return passes + 1


def apply(dst, src, l2p, obs, fuse_diagonal: bool = False) -> int:
    """dst := H src for a Pauli sum over LOGICAL qubits (observable.PauliSum or what it accepts); what dst held does not
    matter, src is only read.  `fuse_diagonal`: the Z-only terms go through ONE diagonal pass whatever their number, when
    there are at least DIAGONAL_MIN_TERMS of them (`plan`).  Returns the HBM passes made."""
    return apply_planned(dst, src, plan(evolution.n_qubits(src, l2p), l2p, obs, fuse_diagonal))


def matrix_elements(ket, bra, l2p, obs) -> np.ndarray:
    """<bra|P_t|ket> (unnormalised, complex128) of every term of a Pauli sum over LOGICAL qubits, WITHOUT its
    coefficient; `bra` may be `ket`."""
    if ket.k != bra.k:
        raise ValueError(f"matrix_elements: chunks of {ket.k} and {bra.k} index bits")
    obs = as_pauli_sum(obs, evolution.n_qubits(ket, l2p))
    x, z = obs.masks(l2p)
    return ket.overlap_pauli(bra, x, z)


def variance(chunk, work, l2p, obs, fuse_diagonal: bool = False) -> float:
    """<psi|H^2|psi> - <psi|H|psi>^2 as norm2(H psi) - <H>^2, unnormalised like every readout here (for a state of norm
    1 it is the energy variance).  `work` := H psi: a second chunk of the same size, overwritten.  `fuse_diagonal`: as
    in `apply`."""
    evolution.check_pair(work, chunk, "variance")
    obs = as_pauli_sum(obs, evolution.n_qubits(chunk, l2p))
    apply(work, chunk, l2p, obs, fuse_diagonal)
    mean = chunk.expectation(obs, l2p=None if l2p is None else list(l2p))
    return work.norm2() - mean * mean


def adjoint_gradient(chunk, work, l2p, rotations, obs) -> tuple[float, np.ndarray]:
    """(E, dE/dtheta) of E(theta) = <psi(theta)|H|psi(theta)>, psi(theta) = R_{n-1} ... R_0 psi_0 with
    R_j = exp(-i theta_j P_j) (no factor 1/2: see the module text), by the adjoint method: one forward run and one
    backward sweep instead of two runs per parameter.

    `rotations`: any form `evolution.as_rotation_arrays` accepts, over LOGICAL qubits; EVERY list entry is its own
    parameter (an angle that appears twice gets two entries: add them).  On entry `chunk` holds psi_0.  The whole list
    is applied forward in one call, E = <psi|H|psi> is read, and `work` := lambda = H psi.  Then for j = n-1 .. 0:
        grad[j] = 2 Im <lambda|P_j|psi>          (with psi = R_j ... R_0 psi_0, lambda = R_{j+1}^+ ... R_{n-1}^+ H psi_{n-1}),
        psi := R_j^+ psi,  lambda := R_j^+ lambda,
    that is one overlap and two single-rotation passes per parameter.  (dE/dtheta_j = 2 Re <psi|H R_{n-1} .. R_{j+1}
    (-i P_j) R_j .. R_0|psi_0> = 2 Re (-i <lambda|P_j|psi>).)  On return `chunk` holds psi_0 again up to rounding and
    `work` is scratch.  E and the gradient are unnormalised, like every readout here."""
    evolution.check_pair(work, chunk, "adjoint_gradient")
    x, z, th = evolution.as_rotation_arrays(rotations)
    if not np.all(np.isfinite(th)):
        raise ValueError("adjoint_gradient: an angle is not finite")
    obs = as_pauli_sum(obs, evolution.n_qubits(chunk, l2p))
    px, pz = evolution.to_physical(x, z, l2p)
    chunk.apply_pauli_rotations(px, pz, th)
    energy = chunk.expectation(obs, l2p=None if l2p is None else list(l2p))
    apply(work, chunk, l2p, obs)
    grad = np.zeros(th.size, dtype=np.float64)
    for j in range(th.size - 1, -1, -1):
        grad[j] = 2.0 * chunk.overlap_pauli(work, px[j:j + 1], pz[j:j + 1])[0].imag
        chunk.apply_pauli_rotations(px[j:j + 1], pz[j:j + 1], -th[j:j + 1])
        work.apply_pauli_rotations(px[j:j + 1], pz[j:j + 1], -th[j:j + 1])
    return float(energy), grad
