"""Pauli rotations on one MI355X: what `qsim_apply_pauli_rotations` costs at 28 and 30 qubits.

    python tools/rotation_probe.py [out.json]          (default: profiles/r14_rotation_probe.json)

Per size, on one `init_random` state, in one process:
  (a) ONE tile pass with 1, 8, 32, 128 and 512 rotations (random strings with X / Y on the index bits 0..10, Z anywhere):
      where the pass stops being bound by HBM and starts being bound by the work on the tile in LDS;
  (b) the same-run yardsticks: one `qsim_apply_1q` (H on qubit 20, one read-modify-write of the state) and one
      `qsim_norm2` (one read);
  (c) one first-order Trotter step of the Heisenberg chain (bonds (q, q + 1): XX, YY, ZZ each) in bond order and in
      brick order (even bonds, then odd), natively and decomposed into gates (`evolution.rotation_gates`: basis changes,
      CNOT ladder, RZ) through `qsim_apply_ops`, whose pass count `qsim_plan_ops` also gives without a device.
Every figure: `warmup` untimed calls, then `reps` timed ones; median, minimum and maximum are kept.  `call_ms` is HIP events
around the whole C call (`time_begin` / `time_end`: for a gate list that includes the host planning of the call, for a
rotation list the upload of the term table), `kernel_ms` the sum of the per-launch events of `qsim_profile_*` over the
same call in a run of its own.  GB/s counts 32 bytes per amplitude and pass (read + write), 16 for `qsim_norm2`.
"""
from __future__ import annotations

import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from quantum_simulations_amd import evolution  # noqa: E402
from quantum_simulations_amd._lib import LIB_PATH, source_hash  # noqa: E402
from quantum_simulations_amd.kernel import planner  # noqa: E402
from quantum_simulations_amd.kernel.device import DeviceChunk, pack_ops  # noqa: E402
from quantum_simulations_amd.observable import PauliSum  # noqa: E402

H_GATE = np.array([[1, 1], [1, -1]], dtype=np.complex128) / np.sqrt(2.0)
COUNTS = (1, 8, 32, 128, 512)


def _stats(ts) -> dict:
    return {"median": statistics.median(ts), "min": min(ts), "max": max(ts)}


def _timed(c: DeviceChunk, fn, warmup: int, reps: int) -> dict:
    """{call_ms, kernel_ms}: events around the call, then (separately) the per-launch events of the profile."""
    for _ in range(warmup):
        fn()
    c.sync()
    call = []
    for _ in range(reps):
        c.time_begin()
        fn()
        call.append(c.time_end())
    kernel = []
    for _ in range(reps):
        c.profile_begin()
        fn()
        kernel.append(sum(e["total_ms"] for e in c.profile_end()))
    return {"call_ms": _stats(call), "kernel_ms": _stats(kernel)}


def tile_pass_rotations(n: int, count: int, seed: int):
    """`count` random rotations that share ONE tile pass: X / Y only on the bits 0..10, Z on any bit."""
    rng = np.random.default_rng(seed)
    x = rng.integers(1, 1 << 11, size=count, dtype=np.uint64)
    z = rng.integers(0, 1 << n, size=count, dtype=np.uint64)
    th = rng.uniform(-np.pi, np.pi, count)
    assert len(planner.plan_pauli_rotations(n, x)[1]) == 1
    return x, z, th


def heisenberg_chain(n: int, brick: bool) -> PauliSum:
    bonds = list(range(n - 1))
    if brick:
        bonds = bonds[0::2] + bonds[1::2]
    return PauliSum([(1.0, {q: p, q + 1: p}) for q in bonds for p in "XYZ"], n_qubits=n)


def probe(n: int, warmup: int, reps: int) -> dict:
    c = DeviceChunk.empty(n)
    rw = 32.0 * (1 << n)
    res = {"n_qubits": n, "state_bytes": rw / 2, "tile_pass": [], "trotter_step": []}
    try:
        c.init_random(1)
        norm2_start = c.norm2()
        # (b) the yardsticks
        t = _timed(c, lambda: c.apply_1q(20, H_GATE), warmup, reps)
        res["apply_1q_h20"] = {**t, "GBps": rw / t["kernel_ms"]["median"] / 1e6}
        t = _timed(c, c.norm2, warmup, reps)
        res["norm2"] = {"call_ms": t["call_ms"], "GBps": rw / 2 / t["call_ms"]["median"] / 1e6}     # (not a profiled class)
        print(json.dumps({k: v for k, v in res.items() if k in ("n_qubits", "apply_1q_h20", "norm2")}), flush=True)
        # (a) one tile pass, more and more rotations
        for count in COUNTS:
            x, z, th = tile_pass_rotations(n, count, 100 + count)
            t = _timed(c, lambda: c.apply_pauli_rotations(x, z, th), warmup, reps)
            assert c.last_rotation_passes == 1
            k_ms = t["kernel_ms"]["median"]
            row = {"rotations": count, "passes": 1, **t, "GBps": rw / k_ms / 1e6, "kernel_us_per_rotation": 1e3 * k_ms / count,
                   "kernel_over_apply_1q": k_ms / res["apply_1q_h20"]["kernel_ms"]["median"]}
            res["tile_pass"].append(row)
            print(json.dumps(row), flush=True)
        # (c) the Heisenberg-chain Trotter step, native against decomposed
        for brick in (False, True):
            x, z, th = evolution.trotter_rotations(heisenberg_chain(n, brick), 0.1)
            ops = [g for xt, zt, tt in zip(x, z, th) for g in evolution.rotation_gates(xt, zt, tt)]
            packed = pack_ops(ops)
            native = _timed(c, lambda: c.apply_pauli_rotations(x, z, th), warmup, reps)
            native_passes = c.last_rotation_passes
            gates = _timed(c, lambda: c.apply_ops(packed), warmup, reps)
            gate_passes = c.apply_ops(packed)
            row = {"order": "brick" if brick else "bond", "rotations": int(len(x)), "gates": len(ops),
                   "native": {"passes": native_passes, "planned_passes": int(len(planner.plan_pauli_rotations(n, x)[1])), **native},
                   "decomposed": {"passes": gate_passes, "planned_passes": planner.pass_count(n, packed), **gates}}
            row["decomposed_over_native_kernel_ms"] = gates["kernel_ms"]["median"] / native["kernel_ms"]["median"]
            row["decomposed_over_native_call_ms"] = gates["call_ms"]["median"] / native["call_ms"]["median"]
            res["trotter_step"].append(row)
            print(json.dumps(row), flush=True)
        res["norm2_end_over_start"] = c.norm2() / norm2_start       # every call above is unitary
    finally:
        c.close()
    return res


def main(out_path: str, warmup: int = 2, reps: int = 7, sizes=(28, 30)) -> dict:
    res = {"tool": "tools/rotation_probe.py", "source_hash": source_hash(), "library": LIB_PATH.name, "warmup": warmup,
           "reps": reps, "sizes": [probe(n, warmup, reps) for n in sizes]}
    Path(out_path).parent.mkdir(parents=True, exist_ok=True)
    Path(out_path).write_text(json.dumps(res, indent=1) + "\n")
    return res


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else str(ROOT / "profiles" / "r14_rotation_probe.json"))
