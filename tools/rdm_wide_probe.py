"""Reduced density matrices of 7 to 12 qubits on one MI355X: what `qsim_reduced_density_matrix_wide` costs at 24, 28 and
30 qubits, next to the r = 6 call of the same run, and what an entanglement entropy costs as a whole.

    python tools/rdm_wide_probe.py [out.json]          (default: profiles/r30_rdm_wide_probe.json)

Per size, on one `init_random` state, in one process (median of `reps` after a warm-up call, HIP events around the whole
call through `time_begin` / `time_end`; the kernel's own ms from the launch profile of one more call): r = 6 through
`qsim_reduced_density_matrix`, r = 7..12 through the wide call, the qubits low (0..r-1), high (the top r bits) and spread
(bit 1, then evenly up to the top bit), as `placements()` of tools/rdm_probe.py.  A call includes the sum over the slices,
the copy of the result (16 * 4^r bytes: 256 MiB at r = 12) and its assembly on the host.  Per row: ms of the call and of
the kernel, `tflops_full` = 8 * 2^(n + r) flop over the CALL's time and `tflops_kernel` over the kernel's, and the ratio
of each to the r = 6 row of the same run and placement (the yardstick: the wide kernel does the same MFMA work per LDS
word and per staged tile).

Then, at every size, `density.entanglement_entropy` of the r = 8, 10, 12 spread sets as a whole call (host clock; the
call ends synchronised) with `numpy.linalg.eigvalsh` on the same matrix timed apart, and once at 24 qubits, r = 8, the
route a user had before: `download` and the numpy restatement of tests/rdm_reference.py.
"""
from __future__ import annotations

import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from quantum_simulations_amd import density  # noqa: E402
from quantum_simulations_amd._lib import LIB_PATH, source_hash  # noqa: E402
from quantum_simulations_amd.kernel.device import DeviceChunk  # noqa: E402
from tools.rdm_probe import placements  # noqa: E402


def _timed(c: DeviceChunk, fn, reps: int) -> float:
    fn()
    ts = []
    for _ in range(reps):
        c.time_begin()
        fn()
        ts.append(c.time_end())
    return statistics.median(ts)


def _kernel_ms(c: DeviceChunk, fn) -> float:
    c.profile_begin()
    fn()
    entries = [e for e in c.profile_end() if e["kernel"].startswith("k_rdm")]
    assert len(entries) == 1 and entries[0]["launches"] == 1, entries
    return entries[0]["total_ms"]


def probe(n: int, reps: int) -> dict:
    c = DeviceChunk.empty(n)
    res = {"n_qubits": n, "state_bytes": 16.0 * (1 << n), "rows": [], "entropy": []}
    try:
        c.init_random(1)
        norm2 = c.norm2()
        base = {}
        for r in range(6, 13):
            call = c.reduced_density_matrix if r == 6 else c.reduced_density_matrix_wide
            for name, qs in placements(n, r).items():
                t_call = _timed(c, lambda: call(qs), reps)
                t_kernel = _kernel_ms(c, lambda: call(qs))
                rho = call(qs)
                flop = 8.0 * (1 << (n + r))
                row = {"r": r, "placement": name, "qubits": qs, "call_ms": t_call, "kernel_ms": t_kernel,
                       "tflops_full": flop / t_call / 1e9, "tflops_kernel": flop / t_kernel / 1e9,
                       "read_GBps_kernel": (1 << max(r - 6, 0)) * 16.0 * (1 << n) / t_kernel / 1e6,
                       "trace_minus_norm2": float(np.trace(rho).real) - norm2,
                       "hermitian": bool(np.array_equal(rho, rho.conj().T))}
                if r == 6:
                    base[name] = row
                row["call_rate_over_r6"] = row["tflops_full"] / base[name]["tflops_full"]
                row["kernel_rate_over_r6"] = row["tflops_kernel"] / base[name]["tflops_kernel"]
                del rho
                res["rows"].append(row)
                print(json.dumps(row), flush=True)
        for r in (8, 10, 12):
            qs = placements(n, r)["spread"]
            density.entanglement_entropy(c, None, qs)                 # warm-up
            t0 = time.perf_counter()
            s = density.entanglement_entropy(c, None, qs)
            whole = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            rho = density.normalised(density.subsystem(c, None, qs))
            matrix = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            np.linalg.eigvalsh(rho)
            eig = (time.perf_counter() - t0) * 1e3
            row = {"r": r, "qubits": qs, "entropy_bits": s, "whole_call_ms": whole, "matrix_ms": matrix, "eigvalsh_ms": eig}
            res["entropy"].append(row)
            print(json.dumps(row), flush=True)
        if n == 24:
            from tests.rdm_reference import rdm_np
            qs = placements(n, 8)["spread"]
            t0 = time.perf_counter()
            psi = c.download()
            down = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            want = rdm_np(psi, qs)
            host = (time.perf_counter() - t0) * 1e3
            got = c.reduced_density_matrix_wide(qs)
            res["download_route_r8"] = {"qubits": qs, "download_ms": down, "rdm_np_ms": host,
                                        "max_abs_difference": float(np.max(np.abs(got - want)))}
            print(json.dumps(res["download_route_r8"]), flush=True)
    finally:
        c.close()
    return res


def main(out_path: str, reps: int = 3) -> dict:
    res = {"tool": "tools/rdm_wide_probe.py", "source_hash": source_hash(), "library": LIB_PATH.name, "reps": reps,
           "sizes": [probe(n, reps) for n in (24, 28, 30)]}
    Path(out_path).parent.mkdir(parents=True, exist_ok=True)
    Path(out_path).write_text(json.dumps(res, indent=1) + "\n")
    return res


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else str(ROOT / "profiles" / "r30_rdm_wide_probe.json"))
