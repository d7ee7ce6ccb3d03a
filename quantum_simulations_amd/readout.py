"""Readout of a chunk whose LOGICAL qubit q lives on index bit l2p[q] (None: identity): the three calls that
`state_calls.StateCalls` makes for `SingleGpuEngine` and `single_node`.  The state does not move: the layout goes into the masks, the qubit lists
and the sampled indices (`observable.PauliSum.masks`, `sampling.to_logical`)."""
from __future__ import annotations

import numpy as np

from quantum_simulations_amd import sampling
from quantum_simulations_amd.observable import as_pauli_sum


def _layout(chunk, l2p) -> list:
    return list(range(chunk.k)) if l2p is None else list(l2p)


# Z-only terms from which `expectation(fuse_diagonal=True)` sends them through `expectation_z_terms` (one read-only pass
# more, whatever their number) instead of leaving them in the per-term passes of `expectation_pauli`.
# MEASURED (profiles/r28_zterm_probe.json, `fused_expectation` and `crossover`): inside the Heisenberg and inside the
# transverse-field Ising chain, at 28 and 30 qubits, fusing wins at every count measured, 1, 2, 4 ... 64: with ONE Z-only
# term 32.8 against 36.7 ms (Heisenberg) and 21.0 against 21.3 ms (Ising) at 30 qubits, 7.4 against 8.6 and 4.99 against
# 5.07 ms at 28 (each outside the spread of its three runs); with 64 terms 2.5 x and 3.5 x.  A Z-only term costs the
# per-term call more than the 2.6 ms pass (0.7 ms at 28 qubits) that takes all of them.
Z_TERMS_MIN = 1


def term_expectations(chunk, x, z, fuse_diagonal: bool = False) -> np.ndarray:
    """<psi|P_t|psi> (unnormalised, float64, in list order) of Pauli strings given as masks over PHYSICAL index bits.
    With `fuse_diagonal` the Z-only strings (x = 0, the identity among them) go through `chunk.expectation_z_terms` when
    there are at least Z_TERMS_MIN of them, the rest through `chunk.expectation_pauli`; the results are merged back in
    list order.  Otherwise everything goes through `expectation_pauli`."""
    x = np.asarray(x, dtype=np.uint64).reshape(-1)
    z = np.asarray(z, dtype=np.uint64).reshape(-1)
    zonly = x == 0
    if not fuse_diagonal or int(np.count_nonzero(zonly)) < max(int(Z_TERMS_MIN), 1):
        return np.asarray(chunk.expectation_pauli(x, z), dtype=np.float64)
    values = np.empty(x.size, dtype=np.float64)
    values[zonly] = chunk.expectation_z_terms(z[zonly])
    if not np.all(zonly):
        values[~zonly] = chunk.expectation_pauli(x[~zonly], z[~zonly])
    return values


def expectation(chunk, l2p, obs, per_term: bool = False, fuse_diagonal: bool = False):
    """<psi|H|psi> (unnormalised) of a Pauli sum over LOGICAL qubits (observable.PauliSum or what it accepts).  With
    `per_term` the array of <psi|P_t|psi> in the sum's term order, without coefficients (`obs.value(values)` is the
    sum).  `fuse_diagonal`: the Z-only terms are evaluated by one Walsh-Hadamard pass (`term_expectations`).  With both
    flags off this is `chunk.expectation`, unchanged."""
    if not per_term and not fuse_diagonal:
        return chunk.expectation(obs, l2p=_layout(chunk, l2p))
    l2p = _layout(chunk, l2p)
    obs = as_pauli_sum(obs, len(l2p))
    values = term_expectations(chunk, *obs.masks(l2p), fuse_diagonal)
    return values if per_term else obs.value(values)


def reduced_density_matrix(chunk, l2p, qubits) -> np.ndarray:
    """Reduced density matrix (unnormalised, complex128 (2^r, 2^r)) of 1 to 6 LOGICAL qubits, bit j of a row or column
    index = qubit qubits[j]."""
    l2p = _layout(chunk, l2p)
    return chunk.reduced_density_matrix([l2p[int(q)] for q in qubits])


def sample(chunk, l2p, shots: int, seed: int = 0, qubits=None) -> np.ndarray:
    """`shots` samples of the register (`sampling.draw(shots, seed)` gives the uniforms): LOGICAL basis-state indices as
    uint64, or with `qubits` the marginal values (bit j = qubit qubits[j])."""
    values = sampling.to_logical(chunk.sample(sampling.draw(shots, seed)), l2p)
    return values if qubits is None else sampling.marginal(values, qubits)
