"""One-GPU runner of dynamic programs (circuit/dynamic.py): mid-circuit measurement, reset and classical control.

The state is one DeviceChunk of n qubits in the identity layout.  The program is cut by `rounds()` into gate segments
and measurement rounds.  A gate segment is ONE `DeviceChunk.apply_ops` call (its conditional gates whose condition is
false left out).  A round reads the joint outcome histogram of its qubits (qsim_probabilities: one read-only pass, 2^r
doubles to the host), draws its outcome and turns the collapse into 2x2 factors that go at the FRONT of the next
segment's op list -- they cost no pass of their own:

    measure, outcome bit b:  |b><b|          reset, outcome bit b:  |0><b|
    sqrt(total / p[m]) folded into the first factor of the round (the state keeps norm 1 over thousands of rounds).

A round at the very end, or directly followed by another round, gets a segment that holds only its factors.

Sampling protocol (tests/dynamic_oracle.py restates it):
    rng = numpy.random.Generator(numpy.random.PCG64(seed)); one u = rng.random() per round, in program order;
    p = probabilities(qubits), total = p.sum(); the outcome is the smallest m with cumsum(p)[m] > u * total.
`forced` gives one outcome per round instead (every branch of a program can be covered); a forced outcome whose
probability p[m] / total is below 1e-12 raises.
"""
from __future__ import annotations

import math
import time
from dataclasses import dataclass, field

import numpy as np

from quantum_simulations_amd.circuit.dynamic import register_value, rounds, validate_dynamic
from quantum_simulations_amd.kernel.device import DeviceChunk
from quantum_simulations_amd.kernel.gates import gate_matrix

MIN_FORCED_PROBABILITY = 1e-12


@dataclass
class RoundRecord:
    qubits: list[int]
    outcome: int            # bit j <-> qubits[j]
    probability: float      # p[outcome] / total
    total: float            # sum of the histogram (the state's norm^2 before the round)


@dataclass
class DynamicResult:
    state: DeviceChunk                      # the caller closes it
    cregs: dict[str, int]                   # register values at the end
    rounds: list[RoundRecord] = field(default_factory=list)
    n_rounds: int = 0
    histogram_launches: int = 0
    fused_passes: int = 0                   # HBM passes of the gate segments (one per op with fused=False)
    device_ms: float | None = None          # event time of every launch (None: a profile was open on the stream already)
    histogram_ms: float | None = None
    host_ms: float = 0.0                    # wall time minus device time


def sample_outcome(p: np.ndarray, u: float) -> int:
    """The smallest m with cumsum(p)[m] > u * p.sum() (zero bins are never chosen; u in [0, 1))."""
    p = np.asarray(p, dtype=np.float64)
    total = p.sum()
    c = np.cumsum(p)
    m = int(np.searchsorted(c, u * total, side="right"))
    if m >= len(p):                          # u * total at or above the last partial sum (rounding): the last bin hit
        m = int(np.flatnonzero(p)[-1])
    return m


def collapse_factors(round_ops: list[dict], qubits: list[int], outcome: int, scale: float) -> list:
    """The round's collapse as (qubits, 2x2) ops: |b><b| for a measure, |0><b| for a reset, `scale` in the first."""
    kind = {op["qubit"]: op["op"] for op in round_ops}
    out = []
    for j, q in enumerate(qubits):
        b = (outcome >> j) & 1
        s = scale if j == 0 else 1.0
        U = np.zeros((2, 2), dtype=np.complex128)
        U[0 if kind[q] == "reset" else b, b] = s
        out.append(([q], U))
    return out


def _gate_op(g: dict, cache: dict):
    """(qubits, matrix); matrices of gates without array parameters are built once per run"""
    try:
        key = (g["gate"], tuple(sorted(g["params"].items())))
        hash(key)
    except TypeError:
        return (list(g["qubits"]), gate_matrix(g["gate"], g["params"]))
    U = cache.get(key)
    if U is None:
        U = cache[key] = gate_matrix(g["gate"], g["params"])
    return (list(g["qubits"]), U)


def run_dynamic(program: dict, seed: int, device: int = 0, forced=None, fused: bool = True) -> DynamicResult:
    """Run a dynamic program from |0...0> on one GPU.  `fused=False` applies every op by its own kernel
    (qsim_apply_ops_unfused): an independent GPU path for cross-checks."""
    prog = validate_dynamic(program)
    n = prog["number_of_qubits"]
    steps = rounds(prog)
    n_rounds = sum(1 for s in steps if s["kind"] == "round")
    if forced is not None and len(forced) != n_rounds:
        raise ValueError(f"forced: {len(forced)} outcomes for {n_rounds} rounds")
    rng = np.random.Generator(np.random.PCG64(seed))
    bits = {name: [0] * size for name, size in prog["cregs"].items()}
    matrices: dict = {}
    chunk = DeviceChunk.zero_state(n, device)
    profiled = False
    try:
        chunk.sync()
        t0 = time.perf_counter()                 # (allocation and |0...0> are not part of the run's times)
        profiled = True
        try:
            chunk.profile_begin()
        except ValueError:
            profiled = False
        res = DynamicResult(state=chunk, cregs={})
        factors: list = []

        def segment(ops):
            if ops:
                res.fused_passes += chunk.apply_ops(ops, fused=fused)

        for step in steps:
            if step["kind"] == "gates":
                ops = [_gate_op(g, matrices) for g in step["ops"]
                       if "condition" not in g or register_value(bits[g["condition"]["creg"]]) == g["condition"]["value"]]
                segment(factors + ops)
                factors = []
                continue
            if factors:                          # the previous round's collapse, before this round reads the state
                segment(factors)
                factors = []
            qubits = step["qubits"]
            p = chunk.probabilities(qubits)
            res.histogram_launches += 1
            total = float(p.sum())
            u = rng.random()
            if forced is not None:
                m = int(forced[len(res.rounds)])
                if not 0 <= m < len(p) or not p[m] / total >= MIN_FORCED_PROBABILITY:
                    raise ValueError(f"round {len(res.rounds)}: forced outcome {m} has probability "
                                     f"{(p[m] / total) if 0 <= m < len(p) else 0.0:.3e} < {MIN_FORCED_PROBABILITY:g}")
            else:
                m = sample_outcome(p, u)
            res.rounds.append(RoundRecord(list(qubits), m, float(p[m] / total), total))
            for op in step["ops"]:
                if op["op"] == "measure":
                    creg, i = op["clbit"]
                    bits[creg][i] = (m >> qubits.index(op["qubit"])) & 1
            factors = collapse_factors(step["ops"], qubits, m, math.sqrt(total / p[m]))
        segment(factors)
        res.n_rounds = len(res.rounds)
        if profiled:
            prof = chunk.profile_end()
            res.device_ms = sum(e["total_ms"] for e in prof)
            res.histogram_ms = sum(e["total_ms"] for e in prof if e["kernel"].startswith("k_hist"))
        else:
            chunk.sync()
        wall_ms = (time.perf_counter() - t0) * 1e3
        res.host_ms = wall_ms - (res.device_ms or 0.0)
        res.cregs = {name: register_value(b) for name, b in bits.items()}
        return res
    except BaseException:
        if profiled:                             # (the profile belongs to the device's stream: never leave it open)
            try:
                chunk.profile_end()
            except Exception:
                pass
        chunk.close()
        raise
