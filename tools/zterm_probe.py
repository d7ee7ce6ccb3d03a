"""Per-term Z expectations on one MI355X: what `qsim_expectation_z_terms` costs at 28 and 30 qubits, next to the calls
that return sums over the same terms and to the per-term call it replaces.

    python tools/zterm_probe.py [out.json] [sizes]    (default: profiles/r28_zterm_probe.json, 28,30)

Per size, on an `init_random` state, in one process:
  (a) `qsim_norm2` (16 B per amplitude), the same-run yardstick;
  (b) the pass with 1 / 8 / 64 / 512 / 2048 / 4096 / 16384 random Z strings: kernel time of the launch profile (the row
      sums are not a profiled class) and HIP events around the whole call; `qsim_diagonal_moments` on the same list, with
      the ratio of the kernel times for lists of up to one pass of terms (a figure to report: above about 1.25 it wants an
      explanation); `qsim_expectation_pauli` on the same list up to 512 terms;
  (c) the all-pairs readout (identity, n singles, n (n - 1) / 2 pairs: 466 terms at 30 qubits), whole call, against
      `qsim_expectation_pauli` on the same list in the same run: `must_hold` is that the new call is faster;
  (d) `readout.expectation(fuse_diagonal=True)` against the plain call for k Z-only terms, k = 1 .. 64, inside the
      Heisenberg chain and inside the transverse-field Ising chain (the threshold forced to 1): the crossover
      `readout.Z_TERMS_MIN` is set from.
Every figure: `warmup` untimed calls, then `reps` timed ones; median, minimum and maximum.
"""
from __future__ import annotations

import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from quantum_simulations_amd import readout  # noqa: E402
from quantum_simulations_amd._lib import LIB_PATH, source_hash  # noqa: E402
from quantum_simulations_amd.kernel.device import DeviceChunk  # noqa: E402
from quantum_simulations_amd.observable import PauliSum  # noqa: E402

COUNTS = (1, 8, 64, 512, 2048, 4096, 16384)
PER_TERM_MAX = 512
ONE_PASS = 2048
Z_COUNTS = (1, 2, 4, 8, 12, 16, 20, 24, 28, 32, 40, 48, 64)
KERNEL = "k_diag_term_values per-term Z expectations"


def _stats(ts) -> dict:
    return {"median": statistics.median(ts), "min": min(ts), "max": max(ts)}


def _timed(c: DeviceChunk, fn, warmup: int, reps: int, kernel: bool = True) -> dict:
    for _ in range(warmup):
        fn()
    c.sync()
    call = []
    for _ in range(reps):
        c.time_begin()
        fn()
        call.append(c.time_end())
    out = {"call_ms": _stats(call)}
    if kernel:
        ms = []
        for _ in range(reps):
            c.profile_begin()
            fn()
            ms.append(sum(e["total_ms"] for e in c.profile_end()))
        out["kernel_ms"] = _stats(ms)
    return out


def _z_terms(n: int, k: int) -> list:
    """k ZZ terms: the bonds of the chain first, then the pairs at distance 2, then 3."""
    pairs = [(q, q + d) for d in (1, 2, 3) for q in range(n - d)]
    return [(1.0, {a: "Z", b: "Z"}) for a, b in pairs[:k]]


def heisenberg_like(n: int, k: int) -> PauliSum:
    return PauliSum([(1.0, {q: p, q + 1: p}) for q in range(n - 1) for p in "XY"] + _z_terms(n, k), n_qubits=n)


def ising_like(n: int, k: int) -> PauliSum:
    return PauliSum([(-1.5, {q: "X"}) for q in range(n)] + _z_terms(n, k), n_qubits=n)


def probe(n: int, warmup: int, reps: int) -> dict:
    amps = float(1 << n)
    res = {"n_qubits": n, "state_bytes": 16.0 * amps, "lists": []}
    c = DeviceChunk.empty(n)
    try:
        c.init_random(1)
        t = _timed(c, c.norm2, warmup, reps, kernel=False)
        res["norm2"] = {**t, "GBps": 16.0 * amps / t["call_ms"]["median"] / 1e6}
        print(json.dumps({"n_qubits": n, "norm2": res["norm2"]}), flush=True)
        # (b)
        for count in COUNTS:
            rng = np.random.default_rng(300 + count)
            z = rng.integers(1, 1 << n, size=count, dtype=np.uint64)
            co = rng.standard_normal(count) / count
            row = {"terms": count}
            row["z_terms"] = {**_timed(c, lambda: c.expectation_z_terms(z), warmup, reps), "passes": c.last_z_terms_passes}
            row["z_terms"]["kernel_GBps"] = 16.0 * amps * c.last_z_terms_passes / row["z_terms"]["kernel_ms"]["median"] / 1e6
            row["diagonal_moments"] = _timed(c, lambda: c.diagonal_moments(z, co), warmup, reps)
            if count <= ONE_PASS:
                row["z_terms_over_moments_kernel_ms"] = row["z_terms"]["kernel_ms"]["median"] / row["diagonal_moments"]["kernel_ms"]["median"]
            if count <= PER_TERM_MAX:
                x0 = np.zeros_like(z)
                r = _timed(c, lambda: c.expectation_pauli(x0, z), warmup, reps)
                row["expectation_pauli"] = {"passes": c.last_expectation_passes, **r}
                row["expectation_pauli_over_z_terms_call_ms"] = r["call_ms"]["median"] / row["z_terms"]["call_ms"]["median"]
            res["lists"].append(row)
            print(json.dumps(row), flush=True)
        # (c)
        z = np.array([0] + [1 << q for q in range(n)] + [(1 << a) | (1 << b) for a in range(n) for b in range(a + 1, n)], dtype=np.uint64)
        x0 = np.zeros_like(z)
        new = _timed(c, lambda: c.expectation_z_terms(z), warmup, reps)
        old = _timed(c, lambda: c.expectation_pauli(x0, z), warmup, reps)
        res["all_pairs_readout"] = {"terms": int(z.size), "z_terms": new, "expectation_pauli": {"passes": c.last_expectation_passes, **old},
                                    "expectation_pauli_over_z_terms_call_ms": old["call_ms"]["median"] / new["call_ms"]["median"],
                                    "must_hold_z_terms_call_is_faster": bool(new["call_ms"]["median"] < old["call_ms"]["median"])}
        print(json.dumps(res["all_pairs_readout"]), flush=True)
        # (d)
        saved = readout.Z_TERMS_MIN
        res["fused_expectation"] = []
        try:
            readout.Z_TERMS_MIN = 1
            for model, build in (("heisenberg", heisenberg_like), ("ising", ising_like)):
                for k in Z_COUNTS:
                    H = build(n, k)
                    x, zz = H.masks(None)
                    row = {"model": model, "z_only_terms": k, "terms": len(H)}
                    for fuse in (False, True):
                        row["fused" if fuse else "plain"] = _timed(c, lambda: readout.term_expectations(c, x, zz, fuse), warmup, reps, kernel=False)
                    row["plain_over_fused_call_ms"] = row["plain"]["call_ms"]["median"] / row["fused"]["call_ms"]["median"]
                    res["fused_expectation"].append(row)
                    print(json.dumps(row), flush=True)
        finally:
            readout.Z_TERMS_MIN = saved
        cross = {}
        for model in ("heisenberg", "ising"):
            rows = [r for r in res["fused_expectation"] if r["model"] == model]
            wins = [r["z_only_terms"] for r in rows if r["plain_over_fused_call_ms"] > 1.0]
            lost = [r["z_only_terms"] for r in rows if r["plain_over_fused_call_ms"] <= 1.0]
            cross[model] = {"fused_wins_at": wins, "loses_at": lost,
                            "smallest_measured_count_that_wins_from_there_on": min([w for w in wins if all(w > l for l in lost)], default=None)}
        res["crossover"] = cross
        print(json.dumps({"crossover": cross, "Z_TERMS_MIN": saved}), flush=True)
    finally:
        c.close()
    return res


def main(out_path: str, warmup: int = 1, reps: int = 3, sizes=(28, 30)) -> dict:
    res = {"tool": "tools/zterm_probe.py", "source_hash": source_hash(), "library": LIB_PATH.name, "warmup": warmup, "reps": reps,
           "Z_TERMS_MIN": readout.Z_TERMS_MIN, "sizes": [probe(n, warmup, reps) for n in sizes]}
    Path(out_path).parent.mkdir(parents=True, exist_ok=True)
    Path(out_path).write_text(json.dumps(res, indent=1) + "\n")
    return res


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else str(ROOT / "profiles" / "r28_zterm_probe.json"),
         sizes=tuple(int(s) for s in sys.argv[2].split(",")) if len(sys.argv) > 2 else (28, 30))
