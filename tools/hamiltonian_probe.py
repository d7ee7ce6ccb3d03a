"""H|psi>, two-state overlaps and one adjoint-gradient step on one MI355X: what `qsim_apply_pauli_sum` and
`qsim_overlap_pauli` cost at 28 and 30 qubits.

    python tools/hamiltonian_probe.py [out.json]          (default: profiles/r18_hamiltonian_probe.json)

Per size, on `init_random` states, in one process:
  (a) the same-run yardsticks: `qsim_copy` (one read and one write of the state: the bytes of a writing pass) and
      `qsim_norm2` (one read: half the bytes of an overlap pass);
  (b) ONE writing tile pass of `qsim_apply_pauli_sum` with 1, 8, 32, 128 and 512 terms (random strings with X / Y on the
      index bits 0..10, Z anywhere), against the copy: where the pass stops being bound by HBM and starts being bound
      by the sum over the tile in LDS;
  (c) a call of TWO tile passes (a writing one and an accumulating one) with 8 and with 128 terms in each; the
      accumulating pass is given as that call minus the writing pass of (b) with the same count -- a difference of two
      medians, named as such;
  (d) ONE tile pass of `qsim_overlap_pauli` with 1, 4, 32 and 256 terms, against `qsim_norm2` and against
      `qsim_expectation_pauli` with the same terms on the same state;
  (e) H of the Heisenberg chain (bonds (q, q + 1): XX, YY, ZZ each) applied once: passes and time;
  (f) one backward step of `hamiltonian.adjoint_gradient`: one overlap with one string and a single-rotation pass on
      each of the two chunks.
Every figure: `warmup` untimed calls, then `reps` timed ones; median, minimum and maximum are kept.  `call_ms` is HIP
events around the whole C call (for the two new calls that includes the upload of the term table, for the overlap and
the other readouts also the row sum and the copy of the results to the host), `kernel_ms` the sum of the per-launch
events of `qsim_profile_*` over the same call in a run of its own (only the classes the profile knows: `qsim_copy`,
`qsim_norm2` and `qsim_expectation_pauli` have none).  GB/s counts 32 bytes per amplitude for a writing pass, a copy and
an overlap pass, 48 for an accumulating pass, 16 for `qsim_norm2`.
"""
from __future__ import annotations

import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from quantum_simulations_amd._lib import LIB_PATH, source_hash  # noqa: E402
from quantum_simulations_amd.kernel.device import DeviceChunk, plan_expectation  # noqa: E402
from quantum_simulations_amd.observable import PauliSum  # noqa: E402

PSUM_COUNTS = (1, 8, 32, 128, 512)
ACC_COUNTS = (8, 128)
OVL_COUNTS = (1, 4, 32, 256)


def _stats(ts) -> dict:
    return {"median": statistics.median(ts), "min": min(ts), "max": max(ts)}


def _timed(c: DeviceChunk, fn, warmup: int, reps: int, profile: bool = True) -> dict:
    """{call_ms[, kernel_ms]}: events around the call, then (separately) the per-launch events of the profile."""
    for _ in range(warmup):
        fn()
    c.sync()
    call = []
    for _ in range(reps):
        c.time_begin()
        fn()
        call.append(c.time_end())
    out = {"call_ms": _stats(call)}
    if profile:
        kernel = []
        for _ in range(reps):
            c.profile_begin()
            fn()
            kernel.append(sum(e["total_ms"] for e in c.profile_end()))
        out["kernel_ms"] = _stats(kernel)
    return out


def tile_pass_terms(n: int, count: int, seed: int, high: bool = False):
    """`count` random strings that share ONE tile pass: X / Y only on the bits 0..10 (high: on the bits 0..2 and 11..18,
    bit 11 always: they cannot share a pass with strings that fill the low 11 bits), Z on any bit; sum |c_t| = 1."""
    rng = np.random.default_rng(seed)
    if high:
        x = (rng.integers(0, 1 << 7, size=count, dtype=np.uint64) << np.uint64(12)) | np.uint64(1 << 11) | rng.integers(0, 8, size=count, dtype=np.uint64)
    else:
        x = rng.integers(1, 1 << 11, size=count, dtype=np.uint64)
        x[0] = 0x7FF
    z = rng.integers(0, 1 << n, size=count, dtype=np.uint64)
    co = rng.uniform(-1.0, 1.0, count)
    return x, z, co / np.sum(np.abs(co))


def heisenberg_chain(n: int) -> PauliSum:
    return PauliSum([(1.0 / (3 * (n - 1)), {q: p, q + 1: p}) for q in range(n - 1) for p in "XYZ"], n_qubits=n)


def probe(n: int, warmup: int, reps: int) -> dict:
    src, dst = DeviceChunk.empty(n), DeviceChunk.empty(n)
    amps = float(1 << n)
    res = {"n_qubits": n, "state_bytes": 16.0 * amps, "psum_writing_pass": [], "psum_two_passes": [], "overlap_pass": []}
    try:
        src.init_random(1)
        dst.init_random(2)
        # (a) the yardsticks
        t = _timed(dst, lambda: dst.copy_from(src), warmup, reps, profile=False)
        copy_ms = t["call_ms"]["median"]
        res["copy"] = {**t, "GBps": 32.0 * amps / copy_ms / 1e6}
        t = _timed(src, src.norm2, warmup, reps, profile=False)
        norm_ms = t["call_ms"]["median"]
        res["norm2"] = {**t, "GBps": 16.0 * amps / norm_ms / 1e6}
        print(json.dumps({k: res[k] for k in ("n_qubits", "copy", "norm2")}), flush=True)
        # (b) one writing tile pass, more and more terms
        writing = {}
        for count in PSUM_COUNTS:
            x, z, co = tile_pass_terms(n, count, 100 + count)
            assert len(plan_expectation(n, x)[1]) == 1
            t = _timed(dst, lambda: dst.apply_pauli_sum(src, x, z, co), warmup, reps)
            assert dst.last_pauli_sum_passes == 1
            k_ms = t["kernel_ms"]["median"]
            writing[count] = k_ms
            row = {"terms": count, "passes": 1, **t, "GBps": 32.0 * amps / k_ms / 1e6, "kernel_us_per_term": 1e3 * k_ms / count,
                   "kernel_over_copy": k_ms / copy_ms, "call_over_copy": t["call_ms"]["median"] / copy_ms}
            res["psum_writing_pass"].append(row)
            print(json.dumps(row), flush=True)
        # (c) a writing and an accumulating pass in one call
        for count in ACC_COUNTS:
            xa, za, ca = tile_pass_terms(n, count, 100 + count)
            xb, zb, cb = tile_pass_terms(n, count, 200 + count, high=True)
            x, z, co = np.concatenate([xa, xb]), np.concatenate([za, zb]), 0.5 * np.concatenate([ca, cb])
            assert [int(v) for v in np.bincount(plan_expectation(n, x)[0])] == [count, count]
            t = _timed(dst, lambda: dst.apply_pauli_sum(src, x, z, co), warmup, reps)
            assert dst.last_pauli_sum_passes == 2
            acc_ms = t["kernel_ms"]["median"] - writing[count]
            row = {"terms_per_pass": count, "passes": 2, **t, "accumulating_pass_ms_by_difference": acc_ms,
                   "accumulating_GBps_by_difference": 48.0 * amps / acc_ms / 1e6, "accumulating_over_writing": acc_ms / writing[count]}
            res["psum_two_passes"].append(row)
            print(json.dumps(row), flush=True)
        # (d) one overlap tile pass against norm2 and against the expectation values of the same strings
        for count in OVL_COUNTS:
            x, z, _ = tile_pass_terms(n, count, 300 + count)
            t = _timed(src, lambda: src.overlap_pauli(dst, x, z), warmup, reps)
            assert src.last_overlap_passes == 1
            e = _timed(src, lambda: src.expectation_pauli(x, z), warmup, reps, profile=False)
            assert src.last_expectation_passes == 1
            k_ms, c_ms = t["kernel_ms"]["median"], t["call_ms"]["median"]
            row = {"terms": count, "passes": 1, **t, "GBps": 32.0 * amps / k_ms / 1e6, "kernel_us_per_term": 1e3 * k_ms / count,
                   "call_over_norm2": c_ms / norm_ms, "expectation_call_ms": e["call_ms"], "call_over_expectation": c_ms / e["call_ms"]["median"]}
            res["overlap_pass"].append(row)
            print(json.dumps(row), flush=True)
        # (e) the Heisenberg chain applied once
        H = heisenberg_chain(n)
        x, z = H.masks(None)
        t = _timed(dst, lambda: dst.apply_pauli_sum(src, x, z, H.coeffs), warmup, reps)
        tiles = [int(v) for v in plan_expectation(n, x)[1]]
        res["heisenberg_chain"] = {"terms": len(H), "passes": dst.last_pauli_sum_passes, "planned_passes": len(tiles),
                                   "terms_per_pass": [int(v) for v in np.bincount(plan_expectation(n, x)[0])], **t,
                                   "kernel_over_copy": t["kernel_ms"]["median"] / copy_ms}
        print(json.dumps(res["heisenberg_chain"]), flush=True)
        # (f) one backward step of the adjoint gradient: <lambda|P|psi>, then exp(+i theta P) on both chunks
        px, pz, th = np.array([3 << 13], dtype=np.uint64), np.array([1 << 13], dtype=np.uint64), np.array([0.37])

        def step():
            src.overlap_pauli(dst, px, pz)
            src.apply_pauli_rotations(px, pz, -th)
            dst.apply_pauli_rotations(px, pz, -th)

        t = _timed(src, step, warmup, reps)
        res["adjoint_backward_step"] = {"overlaps": 1, "rotation_passes": 2, "hbm_bytes": 96.0 * amps, **t,
                                        "GBps": 96.0 * amps / t["kernel_ms"]["median"] / 1e6, "call_over_copy": t["call_ms"]["median"] / copy_ms}
        print(json.dumps(res["adjoint_backward_step"]), flush=True)
    finally:
        src.close()
        dst.close()
    return res


def main(out_path: str, warmup: int = 2, reps: int = 7, sizes=(28, 30)) -> dict:
    res = {"tool": "tools/hamiltonian_probe.py", "source_hash": source_hash(), "library": LIB_PATH.name, "warmup": warmup,
           "reps": reps, "sizes": [probe(n, warmup, reps) for n in sizes]}
    Path(out_path).parent.mkdir(parents=True, exist_ok=True)
    Path(out_path).write_text(json.dumps(res, indent=1) + "\n")
    return res


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else str(ROOT / "profiles" / "r18_hamiltonian_probe.json"))
