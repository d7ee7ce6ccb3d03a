"""Measurement routines of bench.py that need nothing but a chunk: the per-gate sweep and the two streaming ceilings.
`SingleGpuEngine.sweep_gates` / `copy_ceiling` / `stream_ceiling` forward here with the engine's state."""
from __future__ import annotations

import numpy as np

from quantum_simulations_amd.kernel import gates as gate_table
from quantum_simulations_amd.kernel.device import DeviceChunk


def timed(dev: DeviceChunk, fn, reps: int) -> float:
    """Median HIP-event milliseconds of `reps` calls of fn() on the chunk's stream, after one untimed call."""
    fn()
    dev.sync()
    ts = []
    for _ in range(reps):
        dev.time_begin()
        fn()
        ts.append(dev.time_end())
    return float(np.median(ts))


def sweep_gates(state: DeviceChunk, n: int, reps: int = 5) -> dict:
    """BASELINE config 3: one gate per launch on an n-qubit random state, per-target HIP-event
    timing (median of `reps`), as fractions of the 8 TB/s HBM peak of SURVEY 8d's algorithmic bytes:
    H(q) 32 * 2^n for every q; secondary rows T(q), CNOT(q, q+1), CNOT(0, q) at 16 * 2^n.
    Runs on `state` itself when it has n qubits (overwritten: the caller forgets its layout), else on a chunk of its own."""
    dev = state if n == state.k else DeviceChunk.empty(n, state.device)
    dev.init_random(30)
    H, T, CX = gate_table.H(), gate_table.T(), gate_table.CNOT()
    N = 1 << n

    def moved_bytes(fn) -> float:
        """bytes the launch(es) of one gate really move (the library's own per-launch accounting: 32 B per amplitude
        a launch touches -- all of them when a diagonal / control bit lies inside a 128-B line)"""
        dev.profile_begin()
        fn()
        return float(sum(e["hbm_bytes"] for e in dev.profile_end()))

    def row(label, targets, fn, nbytes, note=None) -> dict:
        ms = [timed(dev, lambda q=q: fn(q), reps) for q in targets]
        fr = [nbytes / (t * 1e-3) / 8.0e12 for t in ms]
        moved = [moved_bytes(lambda q=q: fn(q)) for q in targets]
        mf = [b / (t * 1e-3) / 8.0e12 for b, t in zip(moved, ms)]
        out = {"targets": [int(q) for q in targets], "algorithmic_bytes_per_gate": nbytes,
               "ms_per_target": [round(t, 4) for t in ms], "frac_of_8TBps": [round(f, 4) for f in fr],
               # the same launches by the bytes they MOVE: where it exceeds frac_of_8TBps (sub-line control / diagonal
               # bits: every 128-B line moves for half or a quarter of the amplitudes) the algorithmic fraction is
               # at its floor, not the kernel slow
               "moved_bytes_per_target": [int(b) for b in moved], "moved_frac": [round(f, 4) for f in mf],
               "min_frac": round(min(fr), 4), "median_frac": round(float(np.median(fr)), 4),
               "max_frac": round(max(fr), 4), "min_moved_frac": round(min(mf), 4),
               "gate_apps_per_s_median": round(1e3 / float(np.median(ms)), 1)}
        if note:
            out["note"] = note
        return out

    subline = ("a diagonal / control bit below index bit 3 shares every 128-B line with the untouched half: every "
               "line must move, so the algorithmic fraction of those targets is capped near 0.37 by construction")
    rows = {"H(q)": row("H", range(n), lambda q: dev.apply_1q(q, H), 32 * N),
            "T(q)": row("T", range(n), lambda q: dev.apply_1q(q, T), 16 * N, subline),
            "CNOT(q,q+1)": row("CX", range(n - 1), lambda q: dev.apply_2q(q, q + 1, CX), 16 * N, subline),
            "CNOT(0,q)": row("CX0", range(1, n), lambda q: dev.apply_2q(0, q, CX), 16 * N, subline)}
    # the one GEMM-shaped op of the path: dense 2^k x 2^k blocks on the matrix cores (qsim_apply_fused_k -> k_dense_mfma),
    # random unitaries on low / middle / high / mixed index bits above the 128-byte line
    rng = np.random.default_rng(4)
    dense = {}
    MFMA_F64_PEAK_TFLOPS = 78.6     # MI355X dense fp64 matrix peak (MI355X_MICROARCH.md)
    for k in (3, 4, 5, 6):
        mixed = [5, 14, n - 2, n - 9, 8, 12][:k]
        sets = [list(range(3, 3 + k)), list(range(10, 10 + k)), list(range(n - k, n)), mixed, list(range(k))]
        sets = [qs for qs in sets if max(qs) < n and len(set(qs)) == k]
        M = np.linalg.qr(rng.standard_normal((1 << k, 1 << k)) + 1j * rng.standard_normal((1 << k, 1 << k)))[0]
        ms = [timed(dev, lambda qs=qs: dev.apply_fused_k(qs, M), reps) for qs in sets]
        fr = [32 * N / (t * 1e-3) / 8.0e12 for t in ms]
        flop = 8.0 * (1 << k) * N                         # 2^k complex multiply-adds per amplitude
        tf = [flop / (t * 1e-3) / 1e12 for t in ms]
        # which unit bounds the kernel at this size: the matrix cores when the flops at their peak take longer than the
        # bytes at the HBM peak (k = 6: 512 flop per amplitude = 7.0 ms against 4.3 ms at 30 qubits)
        bound = "mfma" if flop / (MFMA_F64_PEAK_TFLOPS * 1e12) > 32.0 * N / 8.0e12 else "hbm"
        dense[f"k={k}"] = {"qubit_sets": sets, "sets_are": ["low", "middle", "high", "mixed", "line bits 0.." + str(k - 1)][:len(sets)],
                           "ms": [round(t, 4) for t in ms], "frac_of_8TBps": [round(f, 4) for f in fr],
                           "flop_per_amplitude": 8 * (1 << k), "achieved_TFLOPs": [round(x, 2) for x in tf],
                           "frac_of_mfma_f64_peak": [round(x / MFMA_F64_PEAK_TFLOPS, 4) for x in tf], "bound": bound,
                           "kernel": f"k_dense_mfma2<{k}> (v_mfma_f64_16x16x4_f64, 16 blocks per wave and step, in place; "
                                     + ("matrix image in LDS" if k >= 5 else "matrix image in registers") + ")"}
    norm2 = dev.norm2()
    if dev is not state:
        dev.close()
    return {"n_qubits": n, "reps": reps, "rows": rows, "dense_blocks": dense, "norm2_after": norm2}


def copy_ceiling(state: DeviceChunk, reps: int = 7) -> dict:
    """Same-run device-to-device copy of a buffer of the state's size (qsim_copy: streaming loads and
    stores, 32 B moved per amplitude): the practical HBM ceiling next to the nominal 8 TB/s."""
    other = DeviceChunk.empty(state.k, state.device)
    ms = timed(other, lambda: other.copy_from(state), reps)
    other.close()
    gbps = 32.0 * (1 << state.k) / (ms * 1e-3) / 1e9
    return {"GBps": round(gbps, 1), "frac_of_8TBps": round(gbps / 8000.0, 4), "ms": round(ms, 4),
            "bytes": 32 * (1 << state.k), "kernel": "k_copy (read + write, non-temporal above 256 MiB)"}


def stream_ceiling(state: DeviceChunk, reps: int = 5) -> dict:
    """What this device streams at the state's size in THIS run: the best of the copy kernel (non-temporal and plain),
    the runtime's device-to-device copy, and an in-place read-modify-write of every amplitude (H on a middle index
    bit: one 32-B round trip per amplitude, the access pattern of the gate kernels themselves).  All move 32 B per
    amplitude.  bench.py reports the fused pass against the best of them (`frac_of_achievable`): unlike the copy
    kernel alone (r04: 0.71 of peak while the in-place H reached 0.77 in the same run) the maximum IS a ceiling of
    what was seen to stream on this box."""
    n = state.k
    other = DeviceChunk.empty(n, state.device)
    nbytes = 32.0 * (1 << n)
    H = gate_table.H()
    other.copy_from(state)
    rows = {"copy_nontemporal": timed(other, lambda: other.copy_from(state, 1), reps),
            "copy_plain": timed(other, lambda: other.copy_from(state, 2), reps),
            "copy_hipMemcpyAsync": timed(other, lambda: other.copy_from(state, 3), reps),
            "inplace_rmw_H_bit12": timed(other, lambda: other.apply_1q(min(12, n - 1), H), reps),
            "inplace_rmw_H_bit5": timed(other, lambda: other.apply_1q(min(5, n - 1), H), reps)}
    other.close()
    gbps = {name: round(nbytes / (ms * 1e-3) / 1e9, 1) for name, ms in rows.items()}
    best = max(gbps, key=gbps.get)
    return {"GBps": gbps[best], "best": best, "frac_of_8TBps": round(gbps[best] / 8000.0, 4), "candidates_GBps": gbps,
            "bytes": int(nbytes), "note": "each candidate moves 32 B per amplitude of a buffer of the state's size; median of %d" % reps}
