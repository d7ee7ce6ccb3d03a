"""TEST INFRASTRUCTURE ONLY -- numpy restatement of a dynamic-program run (runner/dynamic.py's protocol) on the dense
oracle's gates (oracle/dense_oracle.py).  Product code never imports it.

    rng = numpy.random.Generator(numpy.random.PCG64(seed)); one u = rng.random() per round, in program order;
    a round = a maximal run of measure / reset ops, cut into pieces of <= 8 distinct qubits (a repeated qubit starts
    a new piece); p[m] = sum |psi_i|^2 over the i whose bit qubits[j] is bit j of m; total = p.sum(); the outcome is the
    smallest m with cumsum(p)[m] > u * total (or forced[round]).

The collapse is written as a projection (amplitudes that disagree with the outcome set to zero), the renormalisation
psi *= sqrt(total / p[m]), and an X on every reset qubit whose outcome bit is 1 -- not as the runner's 2x2 factors.
`margin` of a round = min over m of |cumsum(p)[m] - u * total|: how far the draw is from changing the outcome.
"""
from __future__ import annotations

import math

import numpy as np

from oracle import dense_oracle as orc

_X = np.array([[0, 1], [1, 0]], dtype=np.complex128)


def _steps(ops):
    steps = []
    for op in ops:
        if op.get("op") not in ("measure", "reset"):
            if not steps or steps[-1][0] != "gates":
                steps.append(("gates", []))
            steps[-1][1].append(op)
            continue
        if not steps or steps[-1][0] != "round" or op["qubit"] in [o["qubit"] for o in steps[-1][1]] or len(steps[-1][1]) == 8:
            steps.append(("round", []))
        steps[-1][1].append(op)
    return steps


def _value(bits):
    return sum(b << i for i, b in enumerate(bits))


def probabilities(psi: np.ndarray, qubits) -> np.ndarray:
    idx = np.arange(len(psi), dtype=np.int64)
    m = np.zeros(len(psi), dtype=np.int64)
    for j, q in enumerate(qubits):
        m |= ((idx >> q) & 1) << j
    return np.bincount(m, weights=np.abs(psi) ** 2, minlength=1 << len(qubits))


def run(program: dict, seed: int, forced=None) -> dict:
    n = program["number_of_qubits"]
    psi = np.zeros(1 << n, dtype=np.complex128)
    psi[0] = 1.0
    rng = np.random.Generator(np.random.PCG64(seed))
    bits = {name: [0] * size for name, size in program["cregs"].items()}
    rounds = []
    for kind, ops in _steps(program["ops"]):
        if kind == "gates":
            for g in ops:
                cond = g.get("condition")
                if cond is not None and _value(bits[cond["creg"]]) != cond["value"]:
                    continue
                name, params, qubits = orc.decode_gate(g)
                U = orc.gate_matrix(name, params)
                if len(qubits) == 1:
                    orc.apply_1q(psi, qubits[0], U)
                else:
                    orc.apply_2q(psi, qubits[0], qubits[1], U)
            continue
        qubits = [o["qubit"] for o in ops]
        p = probabilities(psi, qubits)
        total = p.sum()
        u = rng.random()
        c = np.cumsum(p)
        margin = float(np.min(np.abs(c - u * total)))
        if forced is not None:
            m = int(forced[len(rounds)])
        else:
            hits = np.flatnonzero(c > u * total)
            m = int(hits[0]) if len(hits) else int(np.flatnonzero(p)[-1])
        rounds.append({"qubits": qubits, "outcome": m, "probability": float(p[m] / total), "total": float(total),
                       "margin": margin})
        idx = np.arange(len(psi), dtype=np.int64)
        keep = np.ones(len(psi), dtype=bool)
        for j, q in enumerate(qubits):
            keep &= ((idx >> q) & 1) == ((m >> j) & 1)
        psi[~keep] = 0.0
        psi *= math.sqrt(total / p[m])
        for j, o in enumerate(ops):
            b = (m >> j) & 1
            if o["op"] == "measure":
                creg, i = o["clbit"]
                bits[creg][i] = b
            elif b:
                orc.apply_1q(psi, o["qubit"], _X)
    return {"state": psi, "rounds": rounds, "cregs": {k: _value(v) for k, v in bits.items()}}
