#!/usr/bin/env python3
"""Per-descriptor cost of the fused tile pass: ONE pass holding a complex 2x2 (it takes the factors of the pass, so
every unit-diagonal real 2x2 behind it is lowered to OPC_UNIT1) and M copies of one gate kind (on tile qubit 5, controls on
qubit 9), time vs M -> fixed cost of a pass and slope per gate kind.  Median [min..max] of 7.  M = 120 no longer fits one
pass for the kinds with a matrix ("2p"): the slope over all M then holds a second pass's fixed cost, the one-pass slope
(M = 48 .. 64, both engine bound) does not.
    python tools/gate_cost_probe.py [n_qubits]
OPC_UNIT1 against OPC_REAL1: run it twice on the probe build, one process each,
    QSIM_LIBRARY=quantum_simulations_amd/libqsim_hip_probes.so QSIM_TILE_UNIT=0 | 1 python tools/gate_cost_probe.py
and compare the RY / RY.Z rows (the other kinds do not change)."""
import os
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from quantum_simulations_amd.kernel import gates as gt  # noqa: E402
from quantum_simulations_amd.kernel.device import DeviceChunk  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 28
dev = DeviceChunk.empty(n)
dev.init_random(3)
print(f"# {n} qubits, library {os.path.basename(os.environ.get('QSIM_LIBRARY', 'libqsim_hip.so'))}, QSIM_TILE_UNIT={os.environ.get('QSIM_TILE_UNIT', '(default: on)')}")
host = ([6], gt.T() @ gt.RY(0.7) @ gt.T())
kinds = {"Z": ([5], gt.Z()), "T": ([5], gt.T()), "X": ([5], gt.X()), "H": ([5], gt.H()),
         "RY": ([5], gt.RY(0.3)), "RY.Z": ([5], gt.RY(2.5) @ gt.Z()), "CNOT(9,5)": ([9, 5], gt.CNOT()), "CNOT(20,5)": ([20, 5], gt.CNOT()),
         "CZ(9,5)": ([9, 5], gt.CZ())}
for name, op in kinds.items():
    row = []
    for m in (4, 16, 32, 48, 64, 120):
        ops = [host] + [op] * m
        passes = dev.apply_ops(ops)
        dev.sync()
        ts = []
        for _ in range(7):
            dev.time_begin()
            dev.apply_ops(ops)
            ts.append(dev.time_end())
        row.append((m, passes, float(np.median(ts)), min(ts), max(ts)))
    slope = (row[-1][2] - row[1][2]) / (row[-1][0] - row[1][0])
    one_pass = (row[4][2] - row[3][2]) / (row[4][0] - row[3][0])
    print(f"{name:12s} " + "  ".join(f"M={m}: {t:.3f} [{lo:.3f}..{hi:.3f}] ms ({p}p)" for m, p, t, lo, hi in row) +
          f"   slope {slope * 1e3:.1f} us/gate, M = 48 .. 64: {one_pass * 1e3:.1f}", flush=True)
