#!/usr/bin/env python3
"""Samples for the engine cost table (runner/engine_cost_model.json): random op lists whose targets all lie in ONE tile
with a fast memory pattern (line bits + 3-6, 12-15), so each list is one fused pass whose time past the knee is the gate
engine's.  Every list is planned on the host, its records counted by kind as the engine walks them, and timed on the
device (median of 5, HIP events).  Output: one JSON document for tools/fit_engine_cost_model.py.

    python3 tools/engine_cost_sample.py [n_qubits] [n_lists] [out.json]

The mixes cover the record kinds of the cost table: dense / real / Hadamard 1q, swap and deferred swap, the phase
families and merged runs, lane- and outer-predicated forms, several register groups."""
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
from pass_engine_split import record_kinds  # noqa: E402

from quantum_simulations_amd.kernel import gates as gt  # noqa: E402
from quantum_simulations_amd.kernel.device import DeviceChunk, pack_ops  # noqa: E402

TILE = [0, 1, 2, 3, 4, 5, 6, 12, 13, 14, 15]
OUTSIDE = [20, 23, 9]


def random_list(rng, n_ops):
    """a list of n_ops ops with a random emphasis: each list draws its own weights, so the kinds decorrelate"""
    names = ["H", "RY", "U", "X", "Z", "S", "T", "CXin", "CXout", "CZin", "CZout", "CRin"]
    w = rng.dirichlet(np.full(len(names), 0.6))
    n_targets = int(rng.integers(3, 12))                      # few targets: few register groups
    targets = [int(t) for t in rng.choice(TILE, size=n_targets, replace=False)]
    ops = []
    for _ in range(n_ops):
        kind = names[int(rng.choice(len(names), p=w))]
        t = int(rng.choice(targets))
        c_in = int(rng.choice([q for q in TILE if q != t]))
        c_out = int(rng.choice(OUTSIDE))
        if kind == "H":
            ops.append(([t], gt.H()))
        elif kind == "RY":
            ops.append(([t], gt.RY(float(rng.uniform(0.1, 3.0)))))
        elif kind == "U":
            a = float(rng.uniform(0.1, 3.0))
            ops.append(([t], np.diag([np.exp(-0.5j * a), np.exp(0.5j * a)]) @ gt.RY(float(rng.uniform(0.1, 3.0)))))
        elif kind == "X":
            ops.append(([t], gt.X()))
        elif kind == "Z":
            ops.append(([t], gt.Z()))
        elif kind == "S":
            ops.append(([t], gt.S()))
        elif kind == "T":
            ops.append(([t], gt.T()))
        elif kind == "CXin":
            ops.append(([c_in, t], gt.CNOT()))
        elif kind == "CXout":
            ops.append(([c_out, t], gt.CNOT()))
        elif kind == "CZin":
            ops.append(([c_in, t], gt.CZ()))
        elif kind == "CZout":
            ops.append(([c_out, t], gt.CZ()))
        else:
            ops.append(([c_in, t], np.diag([1, 1, 1, np.exp(1j * float(rng.uniform(0.1, 3.0)))])))
    return ops


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 28
    n_lists = int(sys.argv[2]) if len(sys.argv) > 2 else 160
    out = sys.argv[3] if len(sys.argv) > 3 else str(ROOT / "profile_out" / f"engine_cost_samples_{n}.json")
    rng = np.random.default_rng(20261020)
    dry = out == "--dry"                                       # kinds only (no device): the lists are a function of the seed
    dev = None if dry else DeviceChunk.empty(n)
    if dev:
        dev.init_random(5)
    mask = np.array([sum(1 << b for b in TILE if b >= 3)], dtype=np.uint64)      # the tile is named: the same memory pattern for every list
    rows = []
    for _ in range(n_lists):
        ops = random_list(rng, int(rng.integers(16, 100)))
        packed = pack_ops(ops)
        planned = record_kinds(n, packed, mask)
        if len(planned) != 1:                                  # (over the record budget: two passes)
            continue
        kinds, groups = planned[0]
        if dry:
            rows.append({"kinds": kinds, "groups": groups})
            continue
        dev.apply_ops_tiled(packed, mask)
        dev.sync()
        ts = []
        for _ in range(5):
            dev.time_begin()
            dev.apply_ops_tiled(packed, mask)
            ts.append(dev.time_end())
        rows.append({"ms": float(np.median(ts)), "min_ms": float(min(ts)), "kinds": kinds, "groups": groups})
    if dry:
        json.dump({"n": n, "tile": TILE, "rows": rows}, sys.stdout)
        return
    json.dump({"n": n, "tile": TILE, "rows": rows}, open(out, "w"))
    print(f"{len(rows)} one-pass lists of {n_lists} timed at {n} qubits -> {out}")


if __name__ == "__main__":
    main()
