"""Diagonal Pauli sums on one MI355X: what `qsim_apply_diagonal_phase` and `qsim_diagonal_moments` cost at 28 and 30
qubits, next to the calls they replace.

    python tools/diagonal_probe.py [out.json]          (default: profiles/r22_diagonal_probe.json)

Per size, on one `init_random` state, in one process:
  (a) the same-run yardsticks: `qsim_copy` into a second chunk (32 B per amplitude), one `qsim_apply_1q` (H on qubit 20,
      one read-modify-write) and `qsim_norm2` (16 B);
  (b) the phase pass with 1 / 8 / 64 / 512 / 4096 random Z strings, with the Sherrington-Kirkpatrick instance (all
      n (n - 1) / 2 ZZ pairs) and with a purely high-bit list (every mask on the bits >= 11: one segment holds all 4096
      terms, the worst case of the segmented sum), each next to `qsim_apply_pauli_rotations` on the same list where it has
      at most 512 terms;
  (c) the moments pass on the same lists next to `qsim_expectation_pauli` on the same terms (up to 512);
  (d) one QAOA layer on the SK instance (cost phase + mixer), native against the gate path (`evolution.rotation_gates`
      through `qsim_apply_ops`);
  (e) the first-order Trotter step of the Heisenberg chain with and without `fuse_diagonal`, in bond order (XX, YY, ZZ
      per bond: no run of Z strings) and in letter order (all XX, all YY, all ZZ: one run of n - 1);
  (f) a run of 1 .. 64 Z strings in the middle of a rotation list, as one rotation pass and fused (a pass of its own that
      cuts the rotation pass in two).
Recorded from them: `crossover` (`same_list`: the smallest measured term count from which the diagonal pass beats the
rotation call on the same list; `run_inside_a_list`: the smallest measured run from which fusing wins in (f) -- what
`evolution.DIAGONAL_MIN_RUN` is set from, since `fuse_diagonal` cuts lists), `rate_8_terms_over_copy` (bytes per second of the 8-term phase pass over `qsim_copy`'s; the project's
criterion for a streaming pass is 0.90) and `growth_8_to_4096` (kernel time at 4096 terms over that at 8).
Every figure: `warmup` untimed calls, then `reps` timed ones; median, minimum and maximum.  `call_ms` is HIP events around
the whole C call (it includes the upload of the term tables), `kernel_ms` the per-launch events of `qsim_profile_*` over
the same call in a run of its own (the finishing row sums of the reducing calls are not a profiled class).
"""
from __future__ import annotations

import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from quantum_simulations_amd import diagonal, evolution  # noqa: E402
from quantum_simulations_amd._lib import LIB_PATH, source_hash  # noqa: E402
from quantum_simulations_amd.kernel.device import DeviceChunk, pack_ops  # noqa: E402
from quantum_simulations_amd.observable import PauliSum  # noqa: E402

H_GATE = np.array([[1, 1], [1, -1]], dtype=np.complex128) / np.sqrt(2.0)
COUNTS = (1, 8, 64, 512, 4096)
ROTATION_MAX = 512
RUN_LENGTHS = (1, 8, 16, 20, 24, 28, 32, 48, 64)


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
    rng = np.random.default_rng(7)
    out.append(("high_bits_4096", rng.integers(1, 1 << (n - 11), size=4096, dtype=np.uint64) << np.uint64(11)))
    return out


def heisenberg_chain(n: int) -> PauliSum:
    return PauliSum([(1.0, {q: p, q + 1: p}) for q in range(n - 1) for p in "XYZ"], n_qubits=n)


def probe(n: int, warmup: int, reps: int) -> dict:
    c, other = DeviceChunk.empty(n), DeviceChunk.empty(n)
    amps = float(1 << n)
    rw = 32.0 * amps
    res = {"n_qubits": n, "state_bytes": rw / 2, "phase": [], "moments": []}
    try:
        c.init_random(1)
        norm2_start = c.norm2()
        t = _timed(other, lambda: other.copy_from(c), warmup, reps, kernel=False)
        copy_gbps = rw / t["call_ms"]["median"] / 1e6
        res["copy"] = {**t, "GBps": copy_gbps}
        t = _timed(c, lambda: c.apply_1q(20, H_GATE), warmup, reps)
        res["apply_1q_h20"] = {**t, "GBps": rw / t["kernel_ms"]["median"] / 1e6}
        t = _timed(c, c.norm2, warmup, reps, kernel=False)
        res["norm2"] = {**t, "GBps": rw / 2 / t["call_ms"]["median"] / 1e6}
        print(json.dumps({k: res[k] for k in ("n_qubits", "copy", "apply_1q_h20", "norm2")}), flush=True)
        for name, z in _lists(n):
            rng = np.random.default_rng(int(z.size))
            co = rng.standard_normal(z.size) / z.size
            x0 = np.zeros_like(z)
            t = _timed(c, lambda: c.apply_diagonal_phase(z, co, 0.7), warmup, reps)
            k_ms = t["kernel_ms"]["median"]
            row = {"list": name, "terms": int(z.size), **t, "GBps": rw / k_ms / 1e6, "over_copy": rw / k_ms / 1e6 / copy_gbps,
                   "kernel_over_apply_1q": k_ms / res["apply_1q_h20"]["kernel_ms"]["median"]}
            if z.size <= ROTATION_MAX:
                r = _timed(c, lambda: c.apply_pauli_rotations(x0, z, 0.7 * co), warmup, reps)
                row["rotations"] = {"passes": c.last_rotation_passes, **r}
                row["rotations_over_diagonal_kernel_ms"] = r["kernel_ms"]["median"] / k_ms
            res["phase"].append(row)
            print(json.dumps(row), flush=True)
            t = _timed(c, lambda: c.diagonal_moments(z, co), warmup, reps)
            k_ms = t["kernel_ms"]["median"]
            row = {"list": name, "terms": int(z.size), **t, "GBps": rw / 2 / k_ms / 1e6,
                   "call_over_norm2": t["call_ms"]["median"] / res["norm2"]["call_ms"]["median"]}
            if z.size <= ROTATION_MAX:
                r = _timed(c, lambda: c.expectation_pauli(x0, z), warmup, reps)
                row["expectation_pauli"] = r
                row["expectation_over_moments_call_ms"] = r["call_ms"]["median"] / t["call_ms"]["median"]
            res["moments"].append(row)
            print(json.dumps(row), flush=True)
        # (d) one QAOA layer on the SK instance
        sk = PauliSum([(1.0 / n, {a: "Z", b: "Z"}) for a in range(n) for b in range(a + 1, n)], n_qubits=n)
        native = _timed(c, lambda: diagonal.qaoa(c, None, sk, [0.4], [0.3]), warmup, reps)
        zs, cs = diagonal.diagonal_part(sk)
        ops = [g for zt, ct in zip(zs, cs) for g in evolution.rotation_gates(0, int(zt), 0.4 * float(ct))]
        ops += [g for q in range(n) for g in evolution.rotation_gates(1 << q, 0, 0.3)]
        packed = pack_ops(ops)
        gates = _timed(c, lambda: c.apply_ops(packed), warmup, reps)
        res["qaoa_layer_sk"] = {"cost_terms": len(sk), "native": {"passes": diagonal.qaoa(c, None, sk, [0.4], [0.3]), **native},
                                "gates": {"gates": len(ops), "passes": c.apply_ops(packed), **gates},
                                "gates_over_native_kernel_ms": gates["kernel_ms"]["median"] / native["kernel_ms"]["median"]}
        print(json.dumps(res["qaoa_layer_sk"]), flush=True)
        # (e) the Heisenberg step with and without fuse_diagonal (bond order: XX, YY, ZZ per bond -- no run of Z strings --
        # and letter order: all XX, all YY, all ZZ -- one run of n - 1)
        res["heisenberg_step"] = []
        for order in ("bond", "letter"):
            H = heisenberg_chain(n) if order == "bond" else PauliSum([(1.0, {q: p, q + 1: p}) for p in "XYZ" for q in range(n - 1)], n_qubits=n)
            row = {"order": order, "rotations": len(H)}
            for fuse in (False, True):
                t = _timed(c, lambda: evolution.evolve(c, None, H, 0.1, fuse_diagonal=fuse), warmup, reps)
                row["fused" if fuse else "plain"] = {"passes": evolution.evolve(c, None, H, 0.1, fuse_diagonal=fuse), **t}
            row["plain_over_fused_kernel_ms"] = row["plain"]["kernel_ms"]["median"] / row["fused"]["kernel_ms"]["median"]
            res["heisenberg_step"].append(row)
            print(json.dumps(row), flush=True)
        # (f) a run of L Z strings INSIDE a rotation list (four X / Y rotations of one tile pass on either side, passes that
        # are bound by HBM): fused, the run is a pass of its own and cuts the rotation pass in two
        res["run_inside_a_list"] = []
        saved = evolution.DIAGONAL_MIN_RUN
        try:
            for L in RUN_LENGTHS:
                rng = np.random.default_rng(900 + L)
                x = np.concatenate([rng.integers(1, 1 << 11, size=4, dtype=np.uint64), np.zeros(L, dtype=np.uint64),
                                    rng.integers(1, 1 << 11, size=4, dtype=np.uint64)])
                z = rng.integers(1, 1 << n, size=L + 8, dtype=np.uint64)
                th = rng.uniform(-0.5, 0.5, L + 8)
                row = {"run": L}
                for fuse in (False, True):
                    evolution.DIAGONAL_MIN_RUN = 1 if fuse else saved
                    t = _timed(c, lambda: evolution.apply_rotations(c, None, (x, z, th), fuse_diagonal=fuse), warmup, reps)
                    row["fused" if fuse else "plain"] = {"passes": evolution.apply_rotations(c, None, (x, z, th), fuse_diagonal=fuse), **t}
                row["plain_over_fused_kernel_ms"] = row["plain"]["kernel_ms"]["median"] / row["fused"]["kernel_ms"]["median"]
                res["run_inside_a_list"].append(row)
                print(json.dumps(row), flush=True)
        finally:
            evolution.DIAGONAL_MIN_RUN = saved
        res["norm2_end_over_start"] = c.norm2() / norm2_start       # every call above is unitary or read-only
        # what the issue asks to be recorded
        by = {r["list"]: r for r in res["phase"]}
        beats = [r["terms"] for r in res["phase"] if r["list"].startswith("random_") and "rotations" in r
                 and r["kernel_ms"]["median"] < r["rotations"]["kernel_ms"]["median"]]
        loses = [r["terms"] for r in res["phase"] if r["list"].startswith("random_") and "rotations" in r
                 and r["kernel_ms"]["median"] >= r["rotations"]["kernel_ms"]["median"]]
        wins = [r["run"] for r in res["run_inside_a_list"] if r["plain_over_fused_kernel_ms"] > 1.0]
        lost = [r["run"] for r in res["run_inside_a_list"] if r["plain_over_fused_kernel_ms"] <= 1.0]
        res["crossover"] = {"same_list": {"diagonal_beats_rotations_at": beats, "loses_at": loses,
                                          "smallest_measured_count_that_wins_from_there_on": min([b for b in beats if all(b > l for l in loses)], default=None)},
                            "run_inside_a_list": {"fused_wins_at": wins, "loses_at": lost,
                                                  "smallest_measured_run_that_wins_from_there_on": min([w for w in wins if all(w > l for l in lost)], default=None)}}
        res["rate_8_terms_over_copy"] = by["random_8"]["over_copy"]
        res["meets_0p90"] = bool(by["random_8"]["over_copy"] >= 0.90)
        res["growth_8_to_4096"] = by["random_4096"]["kernel_ms"]["median"] / by["random_8"]["kernel_ms"]["median"]
        print(json.dumps({k: res[k] for k in ("crossover", "rate_8_terms_over_copy", "meets_0p90", "growth_8_to_4096")}), flush=True)
    finally:
        c.close()
        other.close()
    return res


def main(out_path: str, warmup: int = 1, reps: int = 5, sizes=(28, 30)) -> dict:
    res = {"tool": "tools/diagonal_probe.py", "source_hash": source_hash(), "library": LIB_PATH.name, "warmup": warmup,
           "reps": reps, "sizes": [probe(n, warmup, reps) for n in sizes]}
    Path(out_path).parent.mkdir(parents=True, exist_ok=True)
    Path(out_path).write_text(json.dumps(res, indent=1) + "\n")
    return res


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else str(ROOT / "profiles" / "r22_diagonal_probe.json"))
