"""Dynamic programs: circuits that measure or reset qubits before the end and make gates depend on measured bits.

A dynamic program is a dict

    {"number_of_qubits": n, "cregs": {name: size, ...}, "ops": [op, ...]}

where each op is one of
    * a gate dict of the circuit contract (circuit/io.py), optionally with
      "condition": {"creg": name, "value": v} -- the gate runs only when the WHOLE register equals v (OpenQASM 2's
      `if(c==v)`; bit i of the register is clbit i);
    * {"op": "measure", "qubit": q, "clbit": [creg, i]} -- measure q in the computational basis into bit i of creg;
    * {"op": "reset", "qubit": q} -- measure q and bring it to |0>.

`rounds(program)` cuts the op list into gate segments and measurement rounds: a round is a maximal run of measure / reset
ops, cut into pieces of at most MAX_ROUND_QUBITS distinct qubits; a qubit that appears twice in one run starts a new
round.  One round = one joint outcome histogram on the device (qsim_probabilities) and one outcome drawn from it
(runner/dynamic.py).
"""
from __future__ import annotations

from typing import Any

from quantum_simulations_amd.circuit.io import _normalise_gate

MAX_ROUND_QUBITS = 8
_TOP_KEYS = {"number_of_qubits", "cregs", "ops"}


def _is_int(x) -> bool:
    return isinstance(x, int) and not isinstance(x, bool)


def validate_dynamic(program: Any) -> dict:
    """Validate and normalise a dynamic program; raises ValueError on bad input.  Gate ops go through the contract's
    own validation (validate_circuit_dict's per-gate check); the rest is checked here."""
    if not isinstance(program, dict):
        raise ValueError("dynamic program must be a dict")
    missing = _TOP_KEYS - set(program)
    if missing:
        raise ValueError(f"missing required keys: {missing}")
    extra = set(program) - _TOP_KEYS
    if extra:
        raise ValueError(f"unknown top-level keys: {extra}")
    n = program["number_of_qubits"]
    if not _is_int(n) or n < 1:
        raise ValueError(f"number_of_qubits must be positive int, got {n!r}")
    cregs = program["cregs"]
    if not isinstance(cregs, dict):
        raise ValueError("cregs must be a dict {name: size}")
    for name, size in cregs.items():
        if not isinstance(name, str) or not _is_int(size) or size < 1:
            raise ValueError(f"creg {name!r}: size must be a positive int, got {size!r}")
    if not isinstance(program["ops"], list):
        raise ValueError("ops must be a list")
    ops = []
    for i, op in enumerate(program["ops"]):
        where = f"op[{i}]"
        if not isinstance(op, dict):
            raise ValueError(f"{where}: must be a dict")
        if "op" in op:
            kind = op["op"]
            want = {"op", "qubit", "clbit"} if kind == "measure" else {"op", "qubit"} if kind == "reset" else None
            if want is None:
                raise ValueError(f"{where}: unknown op {kind!r} (measure or reset)")
            if set(op) != want:
                raise ValueError(f"{where}: {kind} takes exactly the keys {sorted(want)}")
            q = op["qubit"]
            if not _is_int(q) or not 0 <= q < n:
                raise ValueError(f"{where}: qubit {q!r} out of range [0, {n})")
            if kind == "reset":
                ops.append({"op": "reset", "qubit": q})
                continue
            cb = op["clbit"]
            if (not isinstance(cb, (list, tuple)) or len(cb) != 2 or cb[0] not in cregs or not _is_int(cb[1])
                    or not 0 <= cb[1] < cregs[cb[0]]):
                raise ValueError(f"{where}: clbit must be [creg, index] of a declared register, got {cb!r}")
            ops.append({"op": "measure", "qubit": q, "clbit": [cb[0], cb[1]]})
            continue
        gate = {k: v for k, v in op.items() if k != "condition"}
        g = _normalise_gate(gate, n, i)
        if "condition" in op:
            cond = op["condition"]
            if not isinstance(cond, dict) or set(cond) != {"creg", "value"}:
                raise ValueError(f"{where}: condition must be {{'creg': name, 'value': int}}")
            if cond["creg"] not in cregs:
                raise ValueError(f"{where}: condition on an undeclared register {cond['creg']!r}")
            v = cond["value"]
            if not _is_int(v) or not 0 <= v < (1 << cregs[cond["creg"]]):
                raise ValueError(f"{where}: condition value {v!r} does not fit register {cond['creg']!r}")
            g["condition"] = {"creg": cond["creg"], "value": v}
        ops.append(g)
    return {"number_of_qubits": n, "cregs": dict(cregs), "ops": ops}


def is_measurement(op: dict) -> bool:
    return op.get("op") in ("measure", "reset")


def rounds(program: dict) -> list[dict]:
    """The op list as steps, in program order: {"kind": "gates", "ops": [...]} for a run of gate ops and
    {"kind": "round", "ops": [...], "qubits": [...]} for a measurement round (its measure / reset ops in order and
    their distinct qubits, at most MAX_ROUND_QUBITS).  Rounds cut from one run follow each other directly."""
    steps: list[dict] = []
    for op in program["ops"]:
        if not is_measurement(op):
            if not steps or steps[-1]["kind"] != "gates":
                steps.append({"kind": "gates", "ops": []})
            steps[-1]["ops"].append(op)
            continue
        q = op["qubit"]
        cur = steps[-1] if steps and steps[-1]["kind"] == "round" else None
        if cur is None or q in cur["qubits"] or len(cur["qubits"]) == MAX_ROUND_QUBITS:
            cur = {"kind": "round", "ops": [], "qubits": []}
            steps.append(cur)
        cur["ops"].append(op)
        cur["qubits"].append(q)
    return steps


def register_value(bits: list[int]) -> int:
    """Value of a classical register: bit i of the value = clbit i."""
    return sum(b << i for i, b in enumerate(bits))
