"""Shots from a statevector: the host side of `DeviceChunk.sample` (pure numpy, no device).

The device draws PHYSICAL index values of a chunk, one per uniform the caller hands it (qsim_sample: a two-level inverse
CDF over |amp|^2).  This module makes the uniforms and turns the indices into what a user reads:

    r = draw(shots, seed)                       # numpy.random.Generator(PCG64(seed)), as in runner/dynamic.py
    idx = chunk.sample(r)                       # uint64 physical indices, in the order of r
    y = to_logical(idx, l2p)                    # logical basis states: qubit q = bit q (kernel/ref_dense.simulate)
    m = marginal(y, [3, 0])                     # bit j of m = qubit qubits[j]
    counts(m, 2)                                # {"10": 517, "01": 507}: qiskit order, the LEFTMOST character is the
                                                # highest bit -- the convention of the dense labels in observable.py

`SingleGpuEngine.sample` and `single_node.sample` chain the first four steps.
"""
from __future__ import annotations

import numpy as np


def draw(shots: int, seed: int = 0) -> np.ndarray:
    """`shots` uniforms in [0, 1) from numpy.random.Generator(PCG64(seed)): one per shot, reproducible."""
    if shots < 0:
        raise ValueError(f"draw: {shots} shots")
    return np.random.Generator(np.random.PCG64(seed)).random(int(shots))


def to_logical(indices, l2p=None) -> np.ndarray:
    """Physical index values -> logical ones: bit q of the result = bit l2p[q] of the index (None: identity)."""
    x = np.ascontiguousarray(indices, dtype=np.uint64)
    if l2p is None:
        return x.copy()
    y = np.zeros_like(x)
    for q, p in enumerate(l2p):
        y |= ((x >> np.uint64(p)) & np.uint64(1)) << np.uint64(q)
    return y


def marginal(indices, qubits) -> np.ndarray:
    """Values of the selected qubits: bit j of the result = bit qubits[j] of the index."""
    qubits = [int(q) for q in qubits]
    if len(set(qubits)) != len(qubits) or any(q < 0 or q > 63 for q in qubits):
        raise ValueError(f"marginal: qubits {qubits} repeat or leave 0..63")
    x = np.ascontiguousarray(indices, dtype=np.uint64)
    y = np.zeros_like(x)
    for j, q in enumerate(qubits):
        y |= ((x >> np.uint64(q)) & np.uint64(1)) << np.uint64(j)
    return y


def counts(values, n_bits: int) -> dict:
    """{bitstring: count} of sampled values, `n_bits` characters each, the highest bit first (qiskit order), sorted by
    value."""
    if not 1 <= n_bits <= 64:
        raise ValueError(f"counts: n_bits = {n_bits}")
    v = np.ascontiguousarray(values, dtype=np.uint64).reshape(-1)
    if n_bits < 64 and v.size and int(v.max()) >> n_bits:
        raise ValueError(f"counts: value {int(v.max())} does not fit {n_bits} bits")
    uniq, num = np.unique(v, return_counts=True)
    return {format(int(u), f"0{n_bits}b"): int(c) for u, c in zip(uniq, num)}
