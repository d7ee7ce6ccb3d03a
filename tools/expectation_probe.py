"""Pauli-sum expectation values on one MI355X: what a read of <psi|H|psi> costs at 30 qubits.

    python tools/expectation_probe.py [out.json]

* the sums of the issue -- 1 Z term, 16 mixed terms, MaxCut on K30 (435 ZZ), the Heisenberg chain (87 terms), ~1000
  random terms of weight <= 4, one term wider than a tile -- timed with HIP events around qsim_expectation_pauli
  (median of `reps`), next to qsim_probabilities (r = 8) and qsim_norm2 on the same chunk: ms, passes, GB/s of
  16 B x 2^30 x passes (every pass reads the chunk once);
* a sweep of the terms per tile pass (1 .. 1024 random strings whose X/Y lie in one tile, Z anywhere): where the pass
  stops being bound by HBM.
"""
from __future__ import annotations

import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from quantum_simulations_amd.kernel.device import DeviceChunk  # noqa: E402
from quantum_simulations_amd.observable import PauliSum  # noqa: E402


def _sums(n: int) -> dict:
    rng = np.random.default_rng(7)
    mixed = {}
    for _ in range(16):
        qs = rng.choice(n, size=int(rng.integers(1, 5)), replace=False)
        mixed[" ".join(f"{'XYZ'[int(rng.integers(3))]}{int(q)}" for q in sorted(qs))] = float(rng.standard_normal())
    heis = {}
    for a in range(n - 1):
        for p in "XYZ":
            heis[f"{p}{a} {p}{a + 1}"] = 1.0
    rand = {}
    while len(rand) < 1000:
        qs = rng.choice(n, size=int(rng.integers(1, 5)), replace=False)
        rand[" ".join(f"{'XYZ'[int(rng.integers(3))]}{int(q)}" for q in sorted(qs))] = float(rng.standard_normal())
    return {
        "1 Z term": PauliSum({"Z17": 1.0}, n_qubits=n),
        "16 mixed terms": PauliSum(mixed, n_qubits=n),
        "MaxCut K30: 435 ZZ": PauliSum({f"Z{a} Z{b}": 0.5 for a in range(n) for b in range(a + 1, n)}, n_qubits=n),
        "Heisenberg chain: 87 terms": PauliSum(heis, n_qubits=n),
        "1000 random terms, weight <= 4": PauliSum(rand, n_qubits=n),
        "1 wide term: X on all 30": PauliSum({" ".join(f"X{q}" for q in range(n)): 1.0}, n_qubits=n),
    }


def _timed(c: DeviceChunk, fn, reps: int) -> float:
    fn()
    ts = []
    for _ in range(reps):
        c.time_begin()
        fn()
        ts.append(c.time_end())
    return statistics.median(ts)


def main(out_path: str | None = None, n: int = 30, reps: int = 5) -> dict:
    c = DeviceChunk.zero_state(n)
    nbytes = 16.0 * (1 << n)
    res = {"n_qubits": n, "reps": reps, "sums": [], "terms_per_pass": []}
    try:
        c.init_random(1)
        t_hist = _timed(c, lambda: c.probabilities([0, 4, 9, 13, 18, 22, 26, 29]), reps)
        t_norm = _timed(c, c.norm2, reps)
        res["probabilities_r8_ms"], res["norm2_ms"] = t_hist, t_norm
        res["probabilities_GBps"], res["norm2_GBps"] = nbytes / t_hist / 1e6, nbytes / t_norm / 1e6
        print(json.dumps({k: v for k, v in res.items() if not isinstance(v, list)}), flush=True)
        for name, obs in _sums(n).items():
            x, z = obs.masks()
            ms = _timed(c, lambda: c.expectation_pauli(x, z), reps if len(obs) < 500 else 2)
            passes = c.last_expectation_passes
            row = {"sum": name, "terms": len(obs), "passes": passes, "ms": ms, "ms_per_pass": ms / passes,
                   "GBps": nbytes * passes / ms / 1e6, "rate_vs_probabilities": t_hist * passes / ms,
                   "rate_vs_norm2": t_norm * passes / ms}
            res["sums"].append(row)
            print(json.dumps(row), flush=True)
        rng = np.random.default_rng(3)
        for m in (1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024):
            x = rng.integers(0, 1 << 11, size=m).astype(np.uint64)          # X/Y inside bits 0..10: one tile pass
            z = rng.integers(0, 1 << n, size=m).astype(np.uint64)
            ms = _timed(c, lambda: c.expectation_pauli(x, z), reps)
            row = {"terms": m, "passes": c.last_expectation_passes, "ms": ms, "GBps": nbytes / ms / 1e6,
                   "rate_vs_probabilities": t_hist / ms}
            res["terms_per_pass"].append(row)
            print(json.dumps(row), flush=True)
    finally:
        c.close()
    if out_path:
        Path(out_path).parent.mkdir(parents=True, exist_ok=True)
        Path(out_path).write_text(json.dumps(res, indent=1) + "\n")
    return res


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
