"""Reduced density matrices on one MI355X: what `qsim_reduced_density_matrix` costs at 28 and 30 qubits, next to the
other read-only passes.

    python tools/rdm_probe.py [out.json]          (default: profiles/r13_rdm_probe.json)
    QSIM_LIBRARY=quantum_simulations_amd/libqsim_hip_probes.so QSIM_RDM_FORM=1 python tools/rdm_probe.py \
        profiles/r13_rdm_probe_vector_fma.json    (the A/B partner: r = 4..6 with vector FMAs instead of the matrix cores)

Per size, on one `init_random` state, in one process (median of `reps` after a warm-up call, HIP events around the call
through `time_begin` / `time_end`): `qsim_norm2` once, and for r = 1..6 with the qubits low (0..r-1: line and lane
bits), high (the top r bits) and spread (bit 1, then evenly up to the top bit) `qsim_reduced_density_matrix` and
`qsim_probabilities` on the same qubits.  A call includes the sum over the workgroups' partial matrices and the copy of
the result.  Reported per row: ms, GB/s of the state's bytes, the ratios to `qsim_probabilities` and `qsim_norm2` of
the same run, and the fp64 rate: `tflops_full` counts 8 * 2^r flop per amplitude (every entry of rho, the figure of the
dense k-qubit block), `tflops_done` the flop of the triangle that is computed (per environment index 8 flop per
entry a > b and 4 per diagonal entry; the 4 x 4 blocks on the diagonal compute a few entries more).
"""
from __future__ import annotations

import json
import os
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from quantum_simulations_amd._lib import LIB_PATH, source_hash  # noqa: E402
from quantum_simulations_amd.kernel.device import DeviceChunk  # noqa: E402


def _timed(c: DeviceChunk, fn, reps: int) -> float:
    fn()
    ts = []
    for _ in range(reps):
        c.time_begin()
        fn()
        ts.append(c.time_end())
    return statistics.median(ts)


def placements(n: int, r: int) -> dict:
    spread = [1] + [int(q) for q in np.linspace(4, n - 1, r - 1).round()] if r > 1 else [1]
    return {"low": list(range(r)), "high": list(range(n - r, n)), "spread": spread}


def probe(n: int, reps: int) -> dict:
    c = DeviceChunk.empty(n)
    nbytes = 16.0 * (1 << n)
    res = {"n_qubits": n, "state_bytes": nbytes, "rows": []}
    try:
        c.init_random(1)
        t_norm = _timed(c, c.norm2, reps)
        res.update(norm2_ms=t_norm, norm2_GBps=nbytes / t_norm / 1e6)
        print(json.dumps({k: v for k, v in res.items() if k != "rows"}), flush=True)
        for r in range(1, 7):
            d = 1 << r
            for name, qs in placements(n, r).items():
                t_rdm = _timed(c, lambda: c.reduced_density_matrix(qs), reps)
                t_hist = _timed(c, lambda: c.probabilities(qs), reps)
                rho = c.reduced_density_matrix(qs)
                env = float(1 << (n - r))
                row = {"r": r, "placement": name, "qubits": qs, "rdm_ms": t_rdm, "probabilities_ms": t_hist,
                       "rdm_GBps": nbytes / t_rdm / 1e6, "rdm_over_probabilities": t_rdm / t_hist,
                       "rdm_over_norm2": t_rdm / t_norm,
                       "tflops_full": 8.0 * d * (1 << n) / t_rdm / 1e9,
                       "tflops_done": env * (8.0 * d * (d - 1) / 2 + 4.0 * d) / t_rdm / 1e9,
                       "trace_minus_norm2": float(np.trace(rho).real) - c.norm2(),
                       "max_diagonal_minus_probabilities": float(np.max(np.abs(rho.diagonal().real - c.probabilities(qs))))}
                res["rows"].append(row)
                print(json.dumps(row), flush=True)
    finally:
        c.close()
    return res


def main(out_path: str, reps: int = 5) -> dict:
    # the probe build (QSIM_LIBRARY=.../libqsim_hip_probes.so) with QSIM_RDM_FORM=1 runs r = 4..6 on the vector ALUs
    res = {"tool": "tools/rdm_probe.py", "source_hash": source_hash(), "library": LIB_PATH.name,
           "rdm_form": os.environ.get("QSIM_RDM_FORM", "0") if "probes" in LIB_PATH.name else "0", "reps": reps,
           "sizes": [probe(28, reps), probe(30, reps)]}
    Path(out_path).parent.mkdir(parents=True, exist_ok=True)
    Path(out_path).write_text(json.dumps(res, indent=1) + "\n")
    return res


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else str(ROOT / "profiles" / "r13_rdm_probe.json"))
