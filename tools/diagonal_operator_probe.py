"""Diagonal Pauli sums as operators on one MI355X: what `qsim_apply_diagonal_sum` and `qsim_overlap_diagonal` cost at 28
and 30 qubits, next to the per-term calls they replace, and what `fuse_diagonal` and `qaoa_gradient` gain from them.

    python tools/diagonal_operator_probe.py [out.json] [sizes]    (default: profiles/r24_diagonal_operator_probe.json, 28,30)

Per size, on `init_random` states, in one process:
  (a) the same-run yardsticks: `qsim_copy` into a second chunk (32 B per amplitude) and `qsim_norm2` (16 B);
  (b) the writing pass (32 B), the accumulating pass (48 B), the in-place pass (32 B) and the overlap pass (32 B) with
      1 / 8 / 64 / 512 / 4096 random Z strings and with the Sherrington-Kirkpatrick cost (all n (n - 1) / 2 ZZ pairs), each
      next to the per-term path on the same list where it has at most 512 terms (`qsim_apply_pauli_sum`,
      `qsim_overlap_pauli`); every pass with its bytes per second over `qsim_copy`'s and whether that meets the project's
      0.90 (a figure to report: the ratio moved between rounds);
  (c) `hamiltonian.apply` with and without `fuse_diagonal` (the threshold forced to 1) on the Heisenberg chain and on the
      transverse-field Ising chain with k Z-only terms, k = 2 .. 64 (the ZZ bonds of the chain first, then ZZ pairs at
      distance 2 and 3): the crossover `hamiltonian.DIAGONAL_MIN_TERMS` is set from;
  (d) one Lanczos step (m = 1, with its reorthogonalisation) and one `ground_state` restart (m = 4) of the transverse-field
      Ising chain with and without `fuse_diagonal`, the threshold at the value committed;
  (e) `diagonal.qaoa_gradient` of one SK layer, next to `hamiltonian.adjoint_gradient` on the same circuit written as a
      rotation list (every ZZ pair and every X its own parameter: the path before this call existed), timed once.
Every figure of (a) - (d): `warmup` untimed calls, then `reps` timed ones; median, minimum and maximum.  `call_ms` is HIP
events around the whole call, `kernel_ms` the per-launch events of `qsim_profile_*` over the same call in a run of its own
(the finishing row sums of the reducing calls are not a profiled class).  (e) is wall time of one call, synchronised.
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

from quantum_simulations_amd import diagonal, hamiltonian, krylov  # noqa: E402
from quantum_simulations_amd._lib import LIB_PATH, source_hash  # noqa: E402
from quantum_simulations_amd.kernel.device import DeviceChunk  # noqa: E402
from quantum_simulations_amd.observable import PauliSum  # noqa: E402

COUNTS = (1, 8, 64, 512, 4096)
PER_TERM_MAX = 512
Z_COUNTS = (2, 4, 8, 12, 16, 20, 24, 28, 32, 40, 48, 64)


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


def _lists(n: int) -> list:
    out = []
    for count in COUNTS:
        rng = np.random.default_rng(200 + count)
        out.append((f"random_{count}", rng.integers(1, 1 << n, size=count, dtype=np.uint64)))
    out.append(("sk_all_pairs", np.array([(1 << a) | (1 << b) for a in range(n) for b in range(a + 1, n)], dtype=np.uint64)))
    return out


def _z_terms(n: int, k: int) -> list:
    """k ZZ terms: the bonds of the chain first, then the pairs at distance 2, then 3."""
    pairs = [(q, q + d) for d in (1, 2, 3) for q in range(n - d)]
    return [(1.0, {a: "Z", b: "Z"}) for a, b in pairs[:k]]


def heisenberg_like(n: int, k: int) -> PauliSum:
    return PauliSum([(1.0, {q: p, q + 1: p}) for q in range(n - 1) for p in "XY"] + _z_terms(n, k), n_qubits=n)


def ising_like(n: int, k: int) -> PauliSum:
    return PauliSum([(-1.5, {q: "X"}) for q in range(n)] + _z_terms(n, k), n_qubits=n)


def ising_chain(n: int) -> PauliSum:
    return ising_like(n, n - 1)


def _rate(row: dict, bytes_moved: float, copy_gbps: float) -> None:
    gbps = bytes_moved / row["kernel_ms"]["median"] / 1e6
    row.update({"GBps": gbps, "over_copy": gbps / copy_gbps, "meets_0p90": bool(gbps / copy_gbps >= 0.90)})


def probe(n: int, warmup: int, reps: int) -> dict:
    amps = float(1 << n)
    res = {"n_qubits": n, "state_bytes": 16.0 * amps, "passes": []}
    chunks = [DeviceChunk.empty(n) for _ in range(5)]
    c, other = chunks[0], chunks[1]
    try:
        c.init_random(1)
        other.init_random(2)
        t = _timed(other, lambda: chunks[2].copy_from(c), warmup, reps, kernel=False)
        copy_gbps = 32.0 * amps / t["call_ms"]["median"] / 1e6
        res["copy"] = {**t, "GBps": copy_gbps}
        t = _timed(c, c.norm2, warmup, reps, kernel=False)
        res["norm2"] = {**t, "GBps": 16.0 * amps / t["call_ms"]["median"] / 1e6}
        print(json.dumps({k: res[k] for k in ("n_qubits", "copy", "norm2")}), flush=True)
        # (b) the four passes per list; `other` is rewritten from c after the in-place pass scaled it
        for name, z in _lists(n):
            co = np.random.default_rng(int(z.size)).standard_normal(z.size) / z.size
            x0 = np.zeros_like(z)
            row = {"list": name, "terms": int(z.size)}
            for key, fn, nbytes in (("write", lambda: other.apply_diagonal_sum(c, z, co), 32.0),
                                    ("accumulate", lambda: other.apply_diagonal_sum(c, z, co, accumulate=True), 48.0),
                                    ("in_place", lambda: other.apply_diagonal_sum(other, z, co), 32.0),
                                    ("overlap", lambda: c.overlap_diagonal(other, z, co), 32.0)):
                row[key] = _timed(c, fn, warmup, reps)
                _rate(row[key], nbytes * amps, copy_gbps)
            if z.size <= PER_TERM_MAX:
                r = _timed(c, lambda: other.apply_pauli_sum(c, x0, z, co), warmup, reps)
                row["apply_pauli_sum"] = {"passes": other.last_pauli_sum_passes, **r}
                row["apply_pauli_sum_over_write_kernel_ms"] = r["kernel_ms"]["median"] / row["write"]["kernel_ms"]["median"]
                r = _timed(c, lambda: c.overlap_pauli(other, x0, z), warmup, reps)
                row["overlap_pauli"] = {"passes": c.last_overlap_passes, **r}
                row["overlap_pauli_over_overlap_call_ms"] = r["call_ms"]["median"] / row["overlap"]["call_ms"]["median"]
            res["passes"].append(row)
            print(json.dumps(row), flush=True)
            other.copy_from(c)
        # (c) the crossover of apply(fuse_diagonal=True) inside a mixed sum
        saved = hamiltonian.DIAGONAL_MIN_TERMS
        res["fused_apply"] = []
        try:
            for model, build in (("heisenberg", heisenberg_like), ("ising", ising_like)):
                for k in Z_COUNTS:
                    H = build(n, k)
                    row = {"model": model, "z_only_terms": k, "terms": len(H)}
                    for fuse in (False, True):
                        hamiltonian.DIAGONAL_MIN_TERMS = 1
                        plan = hamiltonian.plan(n, None, H, fuse)
                        t = _timed(c, lambda: hamiltonian.apply_planned(other, c, plan), warmup, reps)
                        row["fused" if fuse else "plain"] = {"passes": hamiltonian.apply_planned(other, c, plan), **t}
                    row["plain_over_fused_kernel_ms"] = row["plain"]["kernel_ms"]["median"] / row["fused"]["kernel_ms"]["median"]
                    res["fused_apply"].append(row)
                    print(json.dumps(row), flush=True)
        finally:
            hamiltonian.DIAGONAL_MIN_TERMS = saved
        cross = {}
        for model in ("heisenberg", "ising"):
            rows = [r for r in res["fused_apply"] if r["model"] == model]
            wins = [r["z_only_terms"] for r in rows if r["plain_over_fused_kernel_ms"] > 1.0]
            lost = [r["z_only_terms"] for r in rows if r["plain_over_fused_kernel_ms"] <= 1.0]
            cross[model] = {"fused_wins_at": wins, "loses_at": lost,
                            "smallest_measured_count_that_wins_from_there_on": min([w for w in wins if all(w > l for l in lost)], default=None)}
        res["crossover"] = cross
        print(json.dumps({"crossover": cross, "DIAGONAL_MIN_TERMS": saved}), flush=True)
        # (d) Lanczos and ground_state on the transverse-field Ising chain, the threshold as committed
        H = ising_chain(n)
        res["krylov_ising"] = {"terms": len(H), "z_only_terms": n - 1, "DIAGONAL_MIN_TERMS": saved}
        for fuse in (False, True):
            def step():
                krylov.lanczos(c, chunks[1:2], None, H, 1, fuse_diagonal=fuse)

            def restart():
                krylov.ground_state(c, chunks[1:5], None, H, m=4, tol=0.0, max_restarts=1, fuse_diagonal=fuse)

            key = "fused" if fuse else "plain"
            res["krylov_ising"][key] = {"lanczos_step": _timed(c, step, warmup, reps), "ground_state_restart_m4": _timed(c, restart, warmup, reps)}
        for what in ("lanczos_step", "ground_state_restart_m4"):
            res["krylov_ising"][f"{what}_plain_over_fused_kernel_ms"] = (res["krylov_ising"]["plain"][what]["kernel_ms"]["median"]
                                                                          / res["krylov_ising"]["fused"][what]["kernel_ms"]["median"])
        print(json.dumps(res["krylov_ising"]), flush=True)
        # (e) the gradient of one SK layer: 2 parameters natively, against n (n - 1) / 2 + n rotation parameters
        sk = PauliSum([(1.0 / n, {a: "Z", b: "Z"}) for a in range(n) for b in range(a + 1, n)], n_qubits=n)
        c.init_random(1)
        diagonal.qaoa_gradient(c, other, None, sk, [0.4], [0.3])
        c.sync()
        t0 = time.perf_counter()
        energy, dg, db = diagonal.qaoa_gradient(c, other, None, sk, [0.4], [0.3])
        c.sync()
        native_ms = (time.perf_counter() - t0) * 1e3
        rot = [({a: "Z", b: "Z"}, 0.4 / n) for a in range(n) for b in range(a + 1, n)] + [({q: "X"}, 0.3) for q in range(n)]
        t0 = time.perf_counter()
        e_rot, grad = hamiltonian.adjoint_gradient(c, other, None, rot, sk)
        c.sync()
        rot_ms = (time.perf_counter() - t0) * 1e3
        zz = n * (n - 1) // 2
        res["qaoa_gradient_sk_layer"] = {
            "cost_terms": len(sk), "native_wall_ms": native_ms, "rotation_list_parameters": len(rot), "rotation_list_wall_ms": rot_ms,
            "rotation_list_over_native": rot_ms / native_ms,
            "dgamma": float(dg[0]), "dgamma_from_rotation_list": float(np.dot(grad[:zz], np.full(zz, 1.0 / n))),
            "dbeta": float(db[0]), "dbeta_from_rotation_list": float(np.sum(grad[zz:])), "energy": energy, "energy_from_rotation_list": e_rot}
        print(json.dumps(res["qaoa_gradient_sk_layer"]), flush=True)
    finally:
        for ch in chunks:
            ch.close()
    return res


def main(out_path: str, warmup: int = 1, reps: int = 3, sizes=(28, 30)) -> dict:
    res = {"tool": "tools/diagonal_operator_probe.py", "source_hash": source_hash(), "library": LIB_PATH.name, "warmup": warmup,
           "reps": reps, "sizes": [probe(n, warmup, reps) for n in sizes]}
    Path(out_path).parent.mkdir(parents=True, exist_ok=True)
    Path(out_path).write_text(json.dumps(res, indent=1) + "\n")
    return res


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else str(ROOT / "profiles" / "r24_diagonal_operator_probe.json"),
         sizes=tuple(int(s) for s in sys.argv[2].split(",")) if len(sys.argv) > 2 else (28, 30))
