"""`qsim_lincomb` against the copy kernel, and what a Lanczos step and a ground-state restart cost, on one MI355X at 28
and 30 qubits.

    python tools/krylov_probe.py [out.json]          (default: profiles/r21_krylov_probe.json)
    python tools/krylov_probe.py --ab [out.json]     (default: profiles/r21_lincomb_ab.json; needs the probe build)

Per size, on `init_random` states, in one process (nine chunks of the state's size: 144 GiB at 30 qubits):
  (a) the same-run yardsticks: `qsim_copy` (32 B per amplitude) and `qsim_norm2` (16 B), HIP events around the call;
  (b) six forms of `qsim_lincomb`, kernel time from the launch profile (class k_lincomb) and events around the call:
      scale (32 B), axpy (48 B), axpy + dot with the bra on the source's neighbour (64 B), 4 sources written (80 B),
      read-only 4 dots (80 B), read-only 1 dot (32 B).  The criterion: bytes per second of the kernel >= 0.90 x the
      copy's of the same run (`over_copy`, `meets_0p90`);
  (c) next to them `qsim_overlap_pauli` with the identity string (32 B: what a dot cost before) and one ACCUMULATING pass
      of `qsim_apply_pauli_sum` with 8 terms (48 B), by difference of a two-pass and a one-pass call as in
      tools/hamiltonian_probe.py;
  (d) m = 8 Lanczos steps (`krylov.lanczos`, full reorthogonalisation) and one restart of `krylov.ground_state(m = 8)`
      on the Heisenberg chain, split by the launch profile into H passes (k_psum) and vector algebra (k_lincomb), with
      the wall time of the call;
  (e) at 28 qubits only: `krylov.ground_state(m = 8, tol = 1e-8)` from a random state to convergence (at most 150
      restarts): H applications, restarts and wall time.
Every timed figure of (a)-(c): `warmup` untimed calls, then `reps` timed ones; median, minimum and maximum are kept.
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

from quantum_simulations_amd import krylov  # noqa: E402
from quantum_simulations_amd._lib import LIB_PATH, source_hash  # noqa: E402
from quantum_simulations_amd.kernel.device import DeviceChunk, plan_expectation  # noqa: E402
from quantum_simulations_amd.observable import PauliSum  # noqa: E402
from tools.hamiltonian_probe import tile_pass_terms  # noqa: E402

M = 8


def _stats(ts) -> dict:
    return {"median": statistics.median(ts), "min": min(ts), "max": max(ts)}


def _timed(c: DeviceChunk, fn, warmup: int, reps: int, kernel: str | None = None) -> dict:
    """{call_ms[, kernel_ms]}: events around the call, then (separately) the per-launch events of class `kernel`."""
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
            ms.append(sum(e["total_ms"] for e in c.profile_end() if e["kernel"].startswith(kernel)))
        out["kernel_ms"] = _stats(ms)
    return out


def heisenberg_chain(n: int) -> PauliSum:
    return PauliSum([(1.0, {q: p, q + 1: p}) for q in range(n - 1) for p in "XYZ"], n_qubits=n)


def _profiled(c: DeviceChunk, fn) -> dict:
    """fn() once under the launch profile: wall time and the time and launches of every kernel class that ran."""
    c.sync()
    c.profile_begin()
    t0 = time.perf_counter()
    out = fn()
    c.sync()
    wall = time.perf_counter() - t0
    classes = {e["kernel"].split()[0]: {"launches": e["launches"], "ms": e["total_ms"], "GBps": e["hbm_bytes"] / e["total_ms"] / 1e6}
               for e in c.profile_end()}
    return {"wall_ms": 1e3 * wall, "classes": classes,
            "h_pass_ms": classes.get("k_psum", {}).get("ms", 0.0), "vector_algebra_ms": classes.get("k_lincomb", {}).get("ms", 0.0)}, out


def forms_probe(dst: DeviceChunk, v: list, warmup: int, reps: int) -> dict:
    """(a) and (b) of the module text on chunks that are already filled: the yardsticks and the six forms."""
    amps = float(len(dst))
    res = {"lincomb": []}
    t = _timed(dst, lambda: dst.copy_from(v[0]), warmup, reps)
    copy_gbps = 32.0 * amps / t["call_ms"]["median"] / 1e6
    res["copy"] = {**t, "GBps": copy_gbps}
    t = _timed(dst, dst.norm2, warmup, reps)
    res["norm2"] = {**t, "GBps": 16.0 * amps / t["call_ms"]["median"] / 1e6}
    print(json.dumps({k: res[k] for k in ("copy", "norm2")}), flush=True)
    co = [0.2 + 0.1j, -0.15j, 0.1, -0.05 + 0.05j]             # (of size < 1: repeated calls do not overflow)
    forms = [("scale", 32, lambda: dst.lincomb(0.999 + 0.01j)),
             ("axpy", 48, lambda: dst.lincomb(1.0, v[:1], co[:1])),
             ("axpy + dot", 64, lambda: dst.lincomb(1.0, v[:1], co[:1], bras=v[1:2])),
             ("4 sources written", 80, lambda: dst.lincomb(0.5, v[:4], co)),
             ("read-only 4 dots", 80, lambda: dst.lincomb(1.0, bras=v[:4])),
             ("read-only 1 dot", 32, lambda: dst.lincomb(1.0, bras=v[:1]))]
    for name, nbytes, fn in forms:
        t = _timed(dst, fn, warmup, reps, kernel="k_lincomb")
        gbps = nbytes * amps / t["kernel_ms"]["median"] / 1e6
        row = {"form": name, "bytes_per_amplitude": nbytes, **t, "GBps": gbps, "over_copy": gbps / copy_gbps,
               "meets_0p90": bool(gbps >= 0.90 * copy_gbps), "call_GBps": nbytes * amps / t["call_ms"]["median"] / 1e6}
        res["lincomb"].append(row)
        print(json.dumps(row), flush=True)
    return res


AB_SETTINGS = [{}, {"QSIM_LC_MAX_WG": "1024"}, {"QSIM_LC_MAX_WG": "2048"}, {"QSIM_LC_MAX_WG": "4096"}, {"QSIM_LC_MAX_WG": "8192"}, {"QSIM_LC_MAX_WG": "16384"},
               {"QSIM_LC_MAX_WG": "1048576"}, {"QSIM_LC_ITEMS": "2"}, {"QSIM_LC_ITEMS": "2", "QSIM_LC_MAX_WG": "4096"},
               {"QSIM_LC_ITEMS": "2", "QSIM_LC_MAX_WG": "16384"}, {}]


def ab_child(n: int, warmup: int = 2, reps: int = 7) -> dict:
    """(a) and (b) under every setting of AB_SETTINGS in ONE process on the same five chunks (the copy kernel's own
    figure moves by 10-20 % between processes with where the allocations land, so settings are only comparable inside
    one); the probe build reads the two knobs at every call.  The first and the last setting are the product's."""
    import os
    res = {"n_qubits": n, "library": LIB_PATH.name, "settings": []}
    chunks = []
    try:
        for j in range(5):
            chunks.append(DeviceChunk.empty(n))
            chunks[-1].init_random(1 + j)
        for knobs in AB_SETTINGS:
            for key in ("QSIM_LC_ITEMS", "QSIM_LC_MAX_WG"):
                os.environ.pop(key, None)
            os.environ.update(knobs)
            res["settings"].append({"knobs": knobs, **forms_probe(chunks[0], chunks[1:], warmup, reps)})
    finally:
        for c in chunks:
            c.close()
    return res


def ab(out_path: str, sizes=(28, 30)) -> dict:
    """`ab_child` per size in a process of its own that loads the probe build."""
    import os
    import subprocess
    env = {**os.environ, "QSIM_LIBRARY": str(LIB_PATH.with_name("libqsim_hip_probes.so"))}
    res = {"tool": "tools/krylov_probe.py --ab", "source_hash": source_hash(), "sizes": []}
    for n in sizes:
        done = subprocess.run([sys.executable, __file__, "--ab-child", str(n)], env=env, capture_output=True, text=True, timeout=400)
        if done.returncode:
            raise RuntimeError(f"n = {n}: exit {done.returncode}\n{done.stderr[-2000:]}")
        row = json.loads(done.stdout.strip().splitlines()[-1])
        for s in row["settings"]:
            print(json.dumps({"n": n, "knobs": s["knobs"], "copy_GBps": round(s["copy"]["GBps"]),
                              "GBps": {r["form"]: round(r["GBps"]) for r in s["lincomb"]}}), flush=True)
        res["sizes"].append(row)
        Path(out_path).parent.mkdir(parents=True, exist_ok=True)
        Path(out_path).write_text(json.dumps(res, indent=1) + "\n")
    return res


def probe(n: int, warmup: int, reps: int) -> dict:
    amps = float(1 << n)
    res = {"n_qubits": n, "state_bytes": 16.0 * amps}
    chunks = []
    try:
        for j in range(M + 1):
            chunks.append(DeviceChunk.empty(n))
            chunks[-1].init_random(1 + j)
        dst, v = chunks[0], chunks[1:]
        res.update(forms_probe(dst, v, warmup, reps))           # (a), (b)
        copy_gbps = res["copy"]["GBps"]
        # (c) what a dot cost before, and an accumulating Pauli-sum pass
        t = _timed(dst, lambda: dst.overlap_pauli(v[0], [0], [0]), warmup, reps, kernel="k_ovl")
        gbps = 32.0 * amps / t["kernel_ms"]["median"] / 1e6
        res["overlap_pauli_identity"] = {**t, "GBps": gbps, "over_copy": gbps / copy_gbps}
        print(json.dumps(res["overlap_pauli_identity"]), flush=True)
        xa, za, ca = tile_pass_terms(n, 8, 108)
        xb, zb, cb = tile_pass_terms(n, 8, 208, high=True)
        x2, z2, c2 = np.concatenate([xa, xb]), np.concatenate([za, zb]), 0.5 * np.concatenate([ca, cb])
        assert [int(q) for q in np.bincount(plan_expectation(n, x2)[0])] == [8, 8]
        one = _timed(dst, lambda: dst.apply_pauli_sum(v[0], xa, za, ca), warmup, reps, kernel="k_psum")
        two = _timed(dst, lambda: dst.apply_pauli_sum(v[0], x2, z2, c2), warmup, reps, kernel="k_psum")
        acc_ms = two["kernel_ms"]["median"] - one["kernel_ms"]["median"]
        gbps = 48.0 * amps / acc_ms / 1e6
        res["psum_accumulating_pass_8_terms"] = {"ms_by_difference": acc_ms, "GBps": gbps, "over_copy": gbps / copy_gbps,
                                                 "writing_pass": one, "two_passes": two}
        print(json.dumps(res["psum_accumulating_pass_8_terms"]), flush=True)
        # (d) Lanczos steps and one restart on the Heisenberg chain
        H = heisenberg_chain(n)
        dst.init_random(99)
        prof, (alphas, betas, k) = _profiled(dst, lambda: krylov.lanczos(dst, v, None, H, M))
        res["lanczos"] = {"m": M, "k": int(k), "terms": len(H), **prof, "per_step": {"h_pass_ms": prof["h_pass_ms"] / k,
                          "vector_algebra_ms": prof["vector_algebra_ms"] / k, "wall_ms": prof["wall_ms"] / k}}
        print(json.dumps(res["lanczos"]), flush=True)
        prof, out = _profiled(dst, lambda: krylov.ground_state(dst, v, None, H, m=M, tol=1e-8, max_restarts=1))
        res["ground_state_one_restart"] = {"m": M, "energy": out[0], "residual": out[1], "h_applications": out[3], **prof}
        print(json.dumps(res["ground_state_one_restart"]), flush=True)
        # (e) to convergence
        if n <= 28:
            dst.init_random(99)
            t0 = time.perf_counter()
            out = krylov.ground_state(dst, v, None, H, m=M, tol=1e-8, max_restarts=150)
            res["ground_state_to_tol"] = {"m": M, "tol": 1e-8, "energy": out[0], "residual": out[1], "restarts": out[2], "h_applications": out[3],
                                          "converged": bool(out[1] <= 1e-8), "wall_s": time.perf_counter() - t0}
            print(json.dumps(res["ground_state_to_tol"]), flush=True)
    finally:
        for c in chunks:
            c.close()
    return res


def main(out_path: str, warmup: int = 2, reps: int = 7, sizes=(28, 30)) -> dict:
    res = {"tool": "tools/krylov_probe.py", "source_hash": source_hash(), "library": LIB_PATH.name, "warmup": warmup,
           "reps": reps, "sizes": []}
    for n in sizes:
        res["sizes"].append(probe(n, warmup, reps))
        Path(out_path).parent.mkdir(parents=True, exist_ok=True)
        Path(out_path).write_text(json.dumps(res, indent=1) + "\n")
    return res


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--ab-child":
        print(json.dumps(ab_child(int(sys.argv[2]))), flush=True)
    elif len(sys.argv) > 1 and sys.argv[1] == "--ab":
        ab(sys.argv[2] if len(sys.argv) > 2 else str(ROOT / "profiles" / "r21_lincomb_ab.json"))
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else str(ROOT / "profiles" / "r21_krylov_probe.json"))
