"""Single-GPU chunked runner with the reference's `run` / `collect_state` interface.

Mirrors wenbo_engine/runner/single_node.py:78-346.  The 2^n state is ONE HBM allocation;
"chunk c" is the window [c*2^k, (c+1)*2^k) of it (block_store.py:14-15), so the reference's
structure -- per step: partner groups first (local ops on the group's chunks, then the
non-local butterflies `apply_1q_pair / apply_2q_pair_* / apply_2q_quad`), then the remaining
chunks -- runs unchanged, minus everything that existed only because chunks lived on disk
(per-step double-buffer directories, fsync, fencing: SURVEY 2 rows 4-5, out of scope).
Step-level checkpoint / resume is opt-in: `checkpoint_every=N` downloads the
state every N steps into `work_dir/state_<a|b>` (the reference's buffer layout, complex128) and
commits it in `work_dir/wal.json` (the reference's document, quantum_simulations_amd/wal.py); a
later `run()` on the same directory and circuit resumes after the last committed step.

`run()` returns an `HbmStateBuffer` (the reference returns the path of the committed buffer
directory); `collect_state()` accepts it and yields the complex128 vector, undoing the staging
permutation when asked, exactly like the reference (single_node.py:326-346).
"""
from __future__ import annotations

import json
import math
from pathlib import Path

import numpy as np

from quantum_simulations_amd.circuit.fusion import batch_levels, split_by_locality
from quantum_simulations_amd.circuit.io import levelize, validate_circuit_dict
from quantum_simulations_amd.circuit.staging import atlas_stages, permute_state
from quantum_simulations_amd.kernel import gpu_nonlocal
from quantum_simulations_amd.kernel.device import DeviceChunk
from quantum_simulations_amd.state_calls import StateCalls

KERNELS = ("hip", "scalar", "batched")  # the reference's names select the same HIP module here


class HbmStateBuffer(StateCalls):
    """Final state of a run: the HBM allocation + its chunk windows; `StateCalls` through the layout `log_to_phys` (set by `run`)."""

    def __init__(self, state: DeviceChunk, chunks: list[DeviceChunk], n_qubits: int,
                 chunk_size: int, work_dir: Path | None):
        self.state, self.chunks = state, chunks
        self.n_qubits, self.chunk_size, self.work_dir = n_qubits, chunk_size, work_dir

    @property
    def l2p(self):
        return getattr(self, "log_to_phys", None) or None

    def apply_observable(self, obs, out=None, fuse_diagonal: bool = False):
        if out is None:                     # (the buffer keeps no second chunk that could be handed back)
            raise ValueError("apply_observable: a buffer has no second chunk of its own; pass `out`")
        return super().apply_observable(obs, out, fuse_diagonal)

    def close(self) -> None:
        for c in self.chunks:
            c.close()
        self.chunks = []
        self.state.close()


def build_steps(cd: dict, k: int, use_fusion: bool, use_staging: bool, staging_method: str):
    """Planner selection of single_node.run (single_node.py:108-121)."""
    if use_staging:  # strict_order: see staging._local_sets_to_steps (reference defect)
        return atlas_stages(cd, k, method=staging_method, strict_order=True)
    levels = levelize(cd)
    if use_fusion:
        return batch_levels(levels, k), None
    steps = []
    for gates in levels:
        if gates:
            local, nonlocal_ = split_by_locality(gates, k)
            steps.append({"local_ops": local, "nonlocal_ops": nonlocal_})
    return steps, None


def _plan_fingerprint(steps, k: int, use_fusion: bool, use_staging: bool, staging_method: str, n_qubits: int | None = None) -> dict:
    """What `done_steps` of a checkpoint refers to: the step list depends on the planner flags, so a
    resumed run must have planned the same steps (qubit lists of every step, hashed)."""
    import hashlib
    h = hashlib.sha256()
    for st in steps:
        for part in ("local_ops", "nonlocal_ops"):
            h.update(repr([list(map(int, qs)) for qs, _ in st[part]]).encode())
            h.update(b"|")
    out = {"k": k, "use_fusion": bool(use_fusion), "use_staging": bool(use_staging),
           "staging_method": staging_method if use_staging else None, "n_steps": len(steps),
           "steps_sha256": h.hexdigest()}
    if n_qubits is not None:
        out["n_qubits"] = int(n_qubits)       # (compared with the committed buffer's manifest on a resume without plan.json)
    return out


def _check_plan_sidecar(work: Path, first_step: int, fingerprint: dict, committed_manifest: dict | None = None) -> None:
    """`done_steps` of a checkpoint indexes the step list of the run that wrote it.  This build records the planner
    flags next to `wal.json` (`plan.json`) and refuses to resume under a different plan.  A checkpoint WITHOUT the
    sidecar was written by the reference (wenbo_engine/runner/single_node.py:78-138 knows no sidecar) or by a round-1
    build: it is accepted only for an unstaged plan -- there both implementations produce the same step list for the
    same `chunk_size` / `use_fusion` (pinned bit-exactly by tests/golden/planner.json), which the caller vouches for by
    passing the flags of the original run -- and the sidecar is written then.  Staged plans differ between the two
    (`strict_order`, wal.py), so a staged resume needs the sidecar."""
    plan_path = work / "plan.json"
    if first_step == 0:
        work.mkdir(parents=True, exist_ok=True)
        plan_path.write_text(json.dumps(fingerprint))
        return
    try:
        saved = json.loads(plan_path.read_text())
    except OSError:
        saved = None
    except ValueError:
        raise ValueError(f"{plan_path} is not valid JSON; refusing to resume")
    if saved is None:
        if fingerprint["use_staging"]:
            raise ValueError(f"checkpoint in {work} has no plan.json (written by the reference or an older build) and this "
                             "run is staged: staged step lists differ between the implementations; refusing to resume")
        if first_step > fingerprint["n_steps"]:
            raise ValueError(f"checkpoint in {work} has {first_step} steps done, this plan has only {fingerprint['n_steps']}")
        # the one planner input the directory itself records: the manifest of the committed buffer holds the chunk_size
        # (and qubit count) the state was written with -- the unstaged step list depends on k = log2(chunk_size), so a
        # resume with another chunk_size would index another step list.  `use_fusion` is recorded nowhere in
        # a reference-written directory and cannot be verified: the caller vouches for it.
        if committed_manifest is not None:
            for key, now in (("chunk_size", 1 << fingerprint["k"]), ("n_qubits", fingerprint.get("n_qubits"))):
                was = committed_manifest.get(key)
                if was is not None and now is not None and int(was) != int(now):
                    raise ValueError(f"checkpoint in {work} was written with {key} = {was}, this run uses {now}: the step "
                                     "lists differ; refusing to resume")
        plan_path.write_text(json.dumps(fingerprint))
        return
    if "n_qubits" not in saved or "n_qubits" not in fingerprint:    # (a sidecar written before the qubit count was recorded)
        saved = {key: v for key, v in saved.items() if key != "n_qubits"}
        fingerprint = {key: v for key, v in fingerprint.items() if key != "n_qubits"}
    if saved != fingerprint:
        raise ValueError(f"checkpoint in {work} was written under a different plan (chunk_size / use_fusion / "
                         f"use_staging / staging_method): saved {saved}, now {fingerprint}; refusing to resume")


def run(circuit_dict: dict, work_dir: str | Path | None = None, chunk_size: int = 1 << 20,
        kernel: str = "hip", use_wal: bool = True, use_fencing: bool = False,
        use_fusion: bool = False, use_staging: bool = False,
        staging_method: str = "heuristic", device: int = 0, checkpoint_every: int = 0,
        checkpoint_dtype: str = "complex128", _stop_after_step: int | None = None) -> HbmStateBuffer:
    """Run the full circuit on HBM-resident chunks.  `use_fencing` is accepted for signature
    compatibility and ignored; `use_wal` matters only together with `checkpoint_every > 0` (see
    the module docstring).  `_stop_after_step` (tests) raises after that step, like the
    reference's WE_CRASH_AFTER_CHUNK crash injection (single_node.py:61-63)."""
    cd = validate_circuit_dict(circuit_dict)
    n = cd["number_of_qubits"]
    N = 1 << n
    chunk_size = min(chunk_size, N)
    if N % chunk_size != 0:
        raise ValueError("2^n must be divisible by chunk_size")
    if kernel not in KERNELS:
        raise ValueError(f"unknown kernel {kernel!r}; this build runs HIP kernels only")
    k = int(math.log2(chunk_size))
    steps, log_to_phys = build_steps(cd, k, use_fusion, use_staging, staging_method)

    work = Path(work_dir) if work_dir is not None else None
    log = None
    first_step = 0
    if checkpoint_every > 0 and use_wal:
        if work is None:
            raise ValueError("checkpoint_every needs a work_dir")
        from quantum_simulations_amd.storage.block_store import load_to_device, write_state
        from quantum_simulations_amd.wal import WAL
        log = WAL(work / "wal.json", circuit_dict=cd)   # raises on a different circuit
        first_step = log.done_steps
        fingerprint = _plan_fingerprint(steps, k, use_fusion, use_staging, staging_method, n_qubits=n)
        committed_manifest = None
        if first_step > 0:
            try:
                from quantum_simulations_amd.storage.block_store import read_manifest
                committed_manifest = read_manifest(work / f"state_{log.committed_buf}")
            except (OSError, ValueError, KeyError):
                committed_manifest = None           # (load_to_device below reports a missing / broken buffer)
        _check_plan_sidecar(work, first_step, fingerprint, committed_manifest)
        first_step = min(first_step, len(steps))
    if first_step > 0:
        state = load_to_device(work / f"state_{log.committed_buf}", device)
        if state.k != n:
            raise ValueError(f"checkpoint holds {state.k} qubits, circuit has {n}")
    else:
        state = DeviceChunk.zero_state(n, device)  # |0..0>: chunk 0, element 0 = 1 (block_store.py:35-65)
    n_chunks = N // chunk_size
    chunks = [state.view(c * chunk_size, k) for c in range(n_chunks)] if n_chunks > 1 else [state]
    stats = {"steps": len(steps), "resumed_from_step": first_step, "hbm_passes": 0, "relayouts": 0,
             "nonlocal_gate_groups": 0, "checkpoints": 0}
    for idx in range(first_step, len(steps)):
        step = steps[idx]
        _apply_step(state, chunks, step["local_ops"], step["nonlocal_ops"], k, stats)
        if log is not None and ((idx + 1) % checkpoint_every == 0 or idx + 1 == len(steps)):
            other = "b" if log.committed_buf == "a" else "a"     # never overwrite the committed buffer
            write_state(work / f"state_{other}", state, chunk_size, dtype=checkpoint_dtype)
            log.commit_step(idx, other)
            stats["checkpoints"] += 1
        if _stop_after_step is not None and idx == _stop_after_step:
            for c in (chunks if n_chunks > 1 else []):
                c.close()
            state.close()
            raise RuntimeError(f"stopped after step {idx} (test crash injection)")

    if work is not None and log_to_phys and log_to_phys != list(range(n)):
        work.mkdir(parents=True, exist_ok=True)
        with open(work / "qubit_mapping.json", "w") as f:  # single_node.py:129-134
            json.dump(log_to_phys, f)
    buf = HbmStateBuffer(state, chunks if n_chunks > 1 else [], n, chunk_size, work)
    buf.log_to_phys = log_to_phys
    buf.stats = stats          # what actually ran: steps, HBM round trips, re-layouts (fusion_stats-style introspection)
    return buf


def _apply_step(state: DeviceChunk, chunks: list[DeviceChunk], local_ops, nonlocal_ops, k: int,
                stats: dict | None = None) -> None:
    """One step.  Local ops use bits < k only, so "every chunk gets the same local pass"
    (_process_local_chunk, single_node.py:208-216) is one launch per op over the whole
    allocation; each chunk still sees local ops before its non-local ones (:253-262)."""
    stats = stats if stats is not None else {"hbm_passes": 0, "relayouts": 0, "nonlocal_gate_groups": 0}
    if local_ops:
        stats["hbm_passes"] += state.apply_ops(local_ops)
    if nonlocal_ops:
        pairs = _relayout_pairs(nonlocal_ops, k)
        if pairs is not None:
            stats["relayouts"] += 1
        else:
            stats["nonlocal_gate_groups"] += 1
        if pairs is not None and len(pairs) <= 3 and min(lo for lo, _ in pairs) < _SUBLINE_BITS:
            # a local bit inside a 128-B line: the slab exchange would touch 16 B of every line
            # (tools/relayout_probe.py: 0.65 TB/s); on ONE allocation the same permutation is a
            # set of SWAP gates between index bits of the whole state = one fused tile pass
            stats["hbm_passes"] += state.apply_ops(nonlocal_ops)
        elif pairs is not None and len(pairs) <= 3:   # a staging SWAP list: ONE all-to-all re-layout
            stats["hbm_passes"] += 1
            gpu_nonlocal.swap_global_local(chunks, [hi - k for _, hi in pairs], [lo for lo, _ in pairs])
        else:
            stats["hbm_passes"] += len(nonlocal_ops)
            _process_nonlocal_groups(chunks, nonlocal_ops, k)


_SWAP_U = None
_SUBLINE_BITS = 3      # index bits 0-2: 8 amplitudes = one 128-B line


def _relayout_pairs(nonlocal_ops, k: int):
    """[(local bit, global bit)] when every op is a SWAP between one local and one non-local qubit
    on pairwise different bits (what staging emits, staging.py:136-152); else None."""
    global _SWAP_U
    if _SWAP_U is None:
        from quantum_simulations_amd.kernel import gates as gate_table
        _SWAP_U = gate_table.SWAP()
    pairs, used = [], set()
    for qs, U in nonlocal_ops:
        if len(qs) != 2 or U.shape != (4, 4) or not np.array_equal(U, _SWAP_U):
            return None
        lo, hi = min(qs), max(qs)
        if not (lo < k <= hi) or lo in used or hi in used:
            return None
        used.update((lo, hi))
        pairs.append((lo, hi))
    return pairs


def _process_nonlocal_groups(chunks, nonlocal_ops, k: int) -> None:
    """Partner groups = chunk indices that agree outside the step's non-local bits
    (single_node.py:219-268)."""
    bits = sorted({q - k for qs, _ in nonlocal_ops for q in qs if q >= k})
    mask = sum(1 << b for b in bits)
    seen: set[int] = set()
    for c in range(len(chunks)):
        base = c & ~mask
        if base in seen:
            continue
        seen.add(base)
        group = {}
        for combo in range(1 << len(bits)):
            idx = base
            for i, b in enumerate(bits):
                if combo >> i & 1:
                    idx |= 1 << b
            group[idx] = chunks[idx]
        for qs, U in nonlocal_ops:
            _apply_nonlocal(group, qs, U, k)


def _apply_nonlocal(data: dict, qs: list[int], U: np.ndarray, k: int) -> None:
    """Dispatch of one non-local gate inside a loaded group (single_node.py:271-321)."""
    def pairs(pbit: int):
        done = set()
        for ci in data:
            c0 = ci & ~(1 << pbit)
            if c0 not in done:
                done.add(c0)
                yield data[c0], data[c0 | (1 << pbit)]

    if len(qs) == 1:
        for c0, c1 in pairs(qs[0] - k):
            gpu_nonlocal.apply_1q_pair(c0, c1, U)
        return
    qa, qb = qs
    if qa < k:
        for c0, c1 in pairs(qb - k):
            gpu_nonlocal.apply_2q_pair_qa_local(c0, c1, qa, U)
    elif qb < k:
        for c0, c1 in pairs(qa - k):
            gpu_nonlocal.apply_2q_pair_qb_local(c0, c1, qb, U)
    else:
        pa, pb = qa - k, qb - k
        done = set()
        for ci in data:
            cb = ci & ~(1 << pa) & ~(1 << pb)
            if cb in done:
                continue
            done.add(cb)
            gpu_nonlocal.apply_2q_quad(data[cb], data[cb | (1 << pb)], data[cb | (1 << pa)],
                                       data[cb | (1 << pa) | (1 << pb)], U)


# ---- the state calls on the final state of `run`: methods of `state_calls.StateCalls` (one docstring each, there) -------------
def expectation(buf: HbmStateBuffer, obs, per_term=False, fuse_diagonal=False):
    """`StateCalls.expectation` on the final state of `run`."""
    return buf.expectation(obs, per_term, fuse_diagonal)


def evolve(buf: HbmStateBuffer, obs, t, steps: int = 1, order: int = 1, fuse_diagonal: bool = False) -> int:
    """`StateCalls.evolve` on the final state of `run`."""
    return buf.evolve(obs, t, steps, order, fuse_diagonal)


def apply_diagonal_phase(buf: HbmStateBuffer, obs, gamma) -> int:
    """`StateCalls.apply_diagonal_phase` on the final state of `run`."""
    return buf.apply_diagonal_phase(obs, gamma)


def diagonal_moments(buf: HbmStateBuffer, obs) -> tuple:
    """`StateCalls.diagonal_moments` on the final state of `run`."""
    return buf.diagonal_moments(obs)


def qaoa(buf: HbmStateBuffer, cost, gammas, betas) -> int:
    """`StateCalls.qaoa` on the final state of `run`."""
    return buf.qaoa(cost, gammas, betas)


def qaoa_gradient(buf: HbmStateBuffer, cost, gammas, betas) -> tuple:
    """`StateCalls.qaoa_gradient` on the final state of `run`; its second chunk lives for the call."""
    return buf.qaoa_gradient(cost, gammas, betas)


def variance(buf: HbmStateBuffer, obs, fuse_diagonal: bool = False) -> float:
    """`StateCalls.variance` on the final state of `run`; its second chunk lives for the call."""
    return buf.variance(obs, fuse_diagonal)


def gradient(buf: HbmStateBuffer, rotations, obs) -> tuple:
    """`StateCalls.gradient` on the final state of `run`; its second chunk lives for the call."""
    return buf.gradient(rotations, obs)


def ground_state(buf: HbmStateBuffer, obs, m: int = 16, tol: float = 1e-8, max_restarts: int = 50, fuse_diagonal: bool = False) -> tuple:
    """`StateCalls.ground_state` from the final state of `run`, which is left normalised in the staging layout."""
    return buf.ground_state(obs, m, tol, max_restarts, fuse_diagonal)


def evolve_krylov(buf: HbmStateBuffer, obs, t, m: int = 16, steps: int = 1, fuse_diagonal: bool = False) -> float:
    """`StateCalls.evolve_krylov` on the final state of `run`."""
    return buf.evolve_krylov(obs, t, m, steps, fuse_diagonal)


def reduced_density_matrix(buf: HbmStateBuffer, qubits) -> np.ndarray:
    """`StateCalls.reduced_density_matrix` of the final state of `run`."""
    return buf.reduced_density_matrix(qubits)


def sample(buf: HbmStateBuffer, shots: int, seed: int = 0, qubits=None) -> np.ndarray:
    """`StateCalls.sample` of the final state of `run`."""
    return buf.sample(shots, seed, qubits)


def collect_state(buf: HbmStateBuffer, apply_permutation: bool = False,
                  work_dir: str | Path | None = None) -> np.ndarray:
    """All chunks back as one complex128 vector; with `apply_permutation` and a
    `qubit_mapping.json` in `work_dir` the staging permutation is undone."""
    state = buf.state.download()
    if apply_permutation and work_dir is not None:
        mapping = Path(work_dir) / "qubit_mapping.json"
        if mapping.exists():
            with open(mapping) as f:
                state = permute_state(state, json.load(f))
    return state
