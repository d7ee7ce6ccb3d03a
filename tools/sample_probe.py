"""Shot sampling on one MI355X: what `qsim_sample` costs at 28 and 30 qubits, next to the other read-only passes.

    python tools/sample_probe.py [out.json]          (default: profiles/r08_sample_probe.json)

Per size, on an `init_random` state, in one run (median of `reps` after a warm-up call):
* `qsim_norm2` and `qsim_probabilities` (r = 8) with HIP events around the call;
* `qsim_sample` for 1, 1024 and 2^20 shots: HIP events around the whole call (`call_ms`: both passes, the copies and the
  host work between them), the host clock around it (`wall_ms`), and from a launch profile of further calls pass A
  (`k_sample_block_sums`) and pass B (`k_sample_resolve`) on their own; `host_and_copies_ms` = call - A - B;
  `locate_ms` = qsim_sample_locate alone on an even block prefix of the same length (the sort by block is part of
  host_and_copies_ms);
* the ratios pass A / norm2 and pass A / probabilities -- pass A moves the bytes of qsim_norm2.
At 30 qubits the acceptance criterion of tests/test_gpu_sampling.py is checked on 64 shots without downloading the state:
the prefix P(i) = sum of |amp|^2 below index i is the sum of qsim_norm2 over the aligned power-of-two views that tile
[0, i) (one per set bit of i; none of the sampling kernels takes part), p_i comes from a one-amplitude download, and
`worst_excess_over_total` = max(P(i) - t, t - P(i + 1), 0) / total over the shots must stay below 1e-12.
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

from quantum_simulations_amd import sampling  # noqa: E402
from quantum_simulations_amd._lib import source_hash  # noqa: E402
from quantum_simulations_amd.kernel.device import DeviceChunk, sample_block_bits, sample_locate  # noqa: E402


def _timed(c: DeviceChunk, fn, reps: int) -> float:
    fn()
    ts = []
    for _ in range(reps):
        c.time_begin()
        fn()
        ts.append(c.time_end())
    return statistics.median(ts)


def _prefix(c: DeviceChunk, end: int) -> np.longdouble:
    """sum of |amp|^2 over [0, end): qsim_norm2 of the aligned views, one per set bit of `end`."""
    total, at = np.longdouble(0), 0
    for b in range(c.k, -1, -1):
        if (end >> b) & 1:
            v = c.view(at, b)
            try:
                total += np.longdouble(v.norm2())
            finally:
                v.close()
            at += 1 << b
    return total


def _criterion(c: DeviceChunk, randnums: np.ndarray, idx: np.ndarray, total: float) -> dict:
    worst = np.longdouble(0)
    zero_weight = 0
    for r, i in zip(randnums, idx):
        i = int(i)
        a = c.download(i, 1)[0]
        p = np.longdouble(a.real) ** 2 + np.longdouble(a.imag) ** 2
        zero_weight += int(p == 0)
        below = _prefix(c, i)
        t = np.longdouble(r) * np.longdouble(total)
        worst = max(worst, below - t, t - (below + p))
    return {"shots_checked": len(idx), "zero_weight_indices": zero_weight,
            "worst_excess_over_total": float(worst / np.longdouble(total)), "tolerance_over_total": 1e-12}


def probe(n: int, reps: int, check_shots: int) -> dict:
    c = DeviceChunk.empty(n)
    nbytes = 16.0 * (1 << n)
    res = {"n_qubits": n, "state_bytes": nbytes, "shots": []}
    try:
        c.init_random(1)
        qs = [q for q in (0, 4, 9, 13, 18, 22, 26, n - 1) if q < n]
        t_norm = _timed(c, c.norm2, reps)
        t_hist = _timed(c, lambda: c.probabilities(qs), reps)
        res.update(norm2_ms=t_norm, probabilities_r8_ms=t_hist, norm2_GBps=nbytes / t_norm / 1e6,
                   probabilities_GBps=nbytes / t_hist / 1e6)
        print(json.dumps({k: v for k, v in res.items() if k != "shots"}), flush=True)
        n_blocks = max(1, (1 << n) >> sample_block_bits())
        even = np.cumsum(np.full(n_blocks, 1.0 / n_blocks))
        for shots in (1, 1024, 1 << 20):
            r = sampling.draw(shots, seed=shots)
            call_ms = _timed(c, lambda: c.sample(r), reps)
            walls, a_ms, b_ms = [], [], []
            for _ in range(reps):
                t0 = time.perf_counter()
                idx = c.sample(r)
                walls.append((time.perf_counter() - t0) * 1e3)
            for _ in range(reps):
                c.profile_begin()
                c.sample(r)
                prof = c.profile_end()
                a_ms.append(sum(e["total_ms"] for e in prof if e["kernel"].startswith("k_sample_block_sums")))
                b_ms.append(sum(e["total_ms"] for e in prof if e["kernel"].startswith("k_sample_resolve")))
            t0 = time.perf_counter()
            sample_locate(even, r)
            locate_ms = (time.perf_counter() - t0) * 1e3
            a, b = statistics.median(a_ms), statistics.median(b_ms)
            row = {"shots": shots, "call_ms": call_ms, "wall_ms": statistics.median(walls), "pass_a_ms": a, "pass_b_ms": b,
                   "host_and_copies_ms": call_ms - a - b, "locate_ms": locate_ms, "passes": c.last_sample_passes,
                   "hit_blocks": int(len(np.unique(idx >> np.uint64(sample_block_bits())))),
                   "pass_a_GBps": nbytes / a / 1e6, "pass_a_over_norm2": a / t_norm, "pass_a_over_probabilities": a / t_hist,
                   "call_over_norm2": call_ms / t_norm}
            res["shots"].append(row)
            print(json.dumps(row), flush=True)
        if check_shots:
            r = sampling.draw(check_shots, seed=99)
            r[:3] = [0.0, np.nextafter(1.0, 0.0), 0.5]
            idx = c.sample(r)
            res["criterion"] = _criterion(c, r, idx, c.norm2())
            res["criterion"]["sample_total_minus_norm2"] = c.last_sample_total - c.norm2()
            print(json.dumps(res["criterion"]), flush=True)
    finally:
        c.close()
    return res


def main(out_path: str, reps: int = 5) -> dict:
    res = {"tool": "tools/sample_probe.py", "source_hash": source_hash(), "reps": reps, "block_bits": sample_block_bits(),
           "sizes": [probe(28, reps, 0), probe(30, reps, 64)]}
    Path(out_path).parent.mkdir(parents=True, exist_ok=True)
    Path(out_path).write_text(json.dumps(res, indent=1) + "\n")
    return res


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else str(ROOT / "profiles" / "r08_sample_probe.json"))
