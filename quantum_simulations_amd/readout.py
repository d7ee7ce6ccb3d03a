"""Readout of a chunk whose LOGICAL qubit q lives on index bit l2p[q] (None: identity): the three calls that
`state_calls.StateCalls` makes for `SingleGpuEngine` and `single_node`.  The state does not move: the layout goes into the masks, the qubit lists
and the sampled indices (`observable.PauliSum.masks`, `sampling.to_logical`)."""
from __future__ import annotations

import numpy as np

from quantum_simulations_amd import sampling


def _layout(chunk, l2p) -> list:
    return list(range(chunk.k)) if l2p is None else list(l2p)


def expectation(chunk, l2p, obs) -> float:
    """<psi|H|psi> (unnormalised) of a Pauli sum over LOGICAL qubits (observable.PauliSum or what it accepts)."""
    return chunk.expectation(obs, l2p=_layout(chunk, l2p))


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
