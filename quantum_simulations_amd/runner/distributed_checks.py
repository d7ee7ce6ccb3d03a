"""What is read out of a partitioned run of the multi-GPU engine (runner/distributed.py), none of it part of the
communication schedule: Pauli-sum expectation values; the self-checks (closed forms over every amplitude, per-shard
fingerprints against a one-device run); the timed BASELINE configurations of bench.py and tools/run_config.py at
N > 1, with the transfer statistics and kernel profiles they print.
"""
from __future__ import annotations

import time

import numpy as np

from quantum_simulations_amd.circuit.staging import permute_state


def _inf_unless_finite(err: float) -> float:
    """A non-finite local error as +inf: what a MAX over ranks (and Python's max) does with a NaN is not defined, +inf
    survives any of them."""
    return err if np.isfinite(err) else float("inf")


class ChecksMixin:
    """For `DistributedEngine`: the shard, the layout (`l2p`), `plan` / `execute`, `_bring_local` and the collectives are there."""

    def norm2(self) -> float:
        self._flush_local()
        return float(self._reduce([self.backend.norm2()])[0])

    def state_vector(self) -> np.ndarray:
        """Whole state in LOGICAL qubit order on every rank (small n only: tests, examples)."""
        self._flush_local()
        parts = self._gather(self.backend.download().view(np.float64).copy())
        return permute_state(np.concatenate([p.view(np.complex128) for p in parts]), self.l2p)


    # ---- observables ------------------------------------------------------------------------------
    def expectation(self, obs) -> float:
        """<psi|H|psi> (unnormalised) of a Pauli sum over LOGICAL qubits (observable.PauliSum or what it accepts).
        Collective: every rank calls it with the same observable and gets the same bits.

        Each term is evaluated on the shards through the current layout: X/Y and Z on local bits by the backend
        (`expectation_pauli`), Z on a rank bit as a per-rank sign.  Terms with X/Y on rank bits are taken in groups of
        one global-X pattern: the re-layout machinery (`_bring_local`: swap-and-stay) first trades those rank bits for
        local bits that carry no X/Y of the group, so each pattern costs one exchange.  The state is NOT moved back:
        the moves are recorded in the layout bookkeeping like any swap-and-stay move (`_dyn`, hence `l2p`), so the
        logical state is unchanged and a following `execute(plan)` finds every qubit where it is.  The per-term shard
        values are all-gathered and added in rank order on every rank, then weighted by the coefficients in term order."""
        from quantum_simulations_amd.observable import as_pauli_sum
        obs = as_pauli_sum(obs, self.n)
        k = self.k
        for t, x in enumerate(obs.x):
            if bin(x).count("1") > k:
                raise ValueError(f"term {obs.labels()[t]!r}: X/Y on {bin(x).count('1')} qubits, a shard holds {k}")
        lo = (1 << k) - 1
        vals = np.zeros(len(obs), dtype=np.float64)
        left = list(range(len(obs)))
        self._flush_local()
        while left:
            xs, zs = obs.masks(self.l2p)
            now = [t for t in left if not int(xs[t]) >> k]
            if now:
                xl = np.array([int(xs[t]) & lo for t in now], dtype=np.uint64)
                zl = np.array([int(zs[t]) & lo for t in now], dtype=np.uint64)
                got = np.asarray(self.backend.expectation_pauli(xl, zl), dtype=np.float64)
                for t, v in zip(now, got):
                    neg = bin(self.rank & (int(zs[t]) >> k)).count("1") & 1
                    vals[t] = -v if neg else v
                left = [t for t in left if t not in set(now)]
                continue
            # one exchange for the global-X pattern of the first term left; the victims carry no X/Y of the group
            pattern = int(xs[left[0]]) >> k
            group = [t for t in left if int(xs[t]) >> k == pattern]
            glob = [k + b for b in range(self.p) if (pattern >> b) & 1]
            busy = 0
            for t in group:
                busy |= int(xs[t]) & lo
            if k - bin(busy).count("1") < len(glob):
                busy = int(xs[left[0]]) & lo          # (too many local X/Y in the group: the first term alone)
            self._bring_local(glob, exclude=[b for b in range(k) if (busy >> b) & 1])
            self._flush_local()
        parts = self._gather(vals)
        total = parts[0].copy()
        for q in parts[1:]:               # (in rank order: every rank adds the same numbers in the same order)
            total = total + q
        return obs.value(total)

    def closed_form_error(self, kind: str) -> float:
        """max over ALL 2^n amplitudes of |amp - closed form| ("ghz" / "ghz_qft"),
        evaluated on every shard in its current (staged) layout and max-reduced over ranks.  Not finite on every rank
        whenever an amplitude of any shard is not finite."""
        self._flush_local()
        local = self.backend.closed_form_error(kind, self.n, self.rank << self.k, self.l2p)
        return self.max_over_ranks(_inf_unless_finite(local))

    def closed_form_sample_error(self, kind: str, windows: int = 16, window: int = 256, seed: int = 7) -> float:
        """The sampled HOST check next to `closed_form_error`: `windows` runs of `window` amplitudes
        of every shard (its first and last run and random ones) are downloaded and compared on the host with the closed
        forms of SURVEY 8c written out in numpy -- an implementation that shares nothing with the device reduction;
        max over the samples of all ranks.  Not finite on every rank whenever a sampled amplitude is not finite."""
        self._flush_local()
        size = 1 << self.k
        window = min(window, size)
        rng = np.random.default_rng(seed + self.rank)
        starts = sorted({0, size - window} | {int(x) for x in rng.integers(0, size - window + 1, size=max(0, windows - 2))})
        l2p = self.l2p
        worst = 0.0
        for start in starts:
            got = self.backend.download(start, window)
            x = (self.rank << self.k) + start + np.arange(window, dtype=np.int64)       # physical index
            y = np.zeros_like(x)                                                          # logical index
            for q, pbit in enumerate(l2p):
                y |= ((x >> pbit) & 1) << q
            if kind == "ghz":
                want = np.where((y == 0) | (y == (1 << self.n) - 1), 2.0 ** -0.5, 0.0).astype(np.complex128)
            elif kind == "ghz_qft":       # psi[y] = 2^-(n+1)/2 (1 + exp(-2 pi i y / 2^n))
                want = 2.0 ** (-(self.n + 1) / 2) * (1.0 + np.exp(-2j * np.pi * (y.astype(np.float64) / 2.0 ** self.n)))
            else:
                raise ValueError("kind must be 'ghz' or 'ghz_qft'")
            worst = max(worst, _inf_unless_finite(float(np.max(np.abs(got - want)))))
        return self.max_over_ranks(worst)

    # ---- amplitude-level check of states too large to gather ------------------------------
    def shard_selectors(self) -> list:
        """(sel_mask, sel_value) per rank: the set of LOGICAL indices rank r holds in the current layout -- the logical
        qubits that sit on rank bits, with the values r gives them (qsim_fingerprint's filter on a one-GPU state)."""
        l2p = self.l2p
        glob = [q for q in range(self.n) if l2p[q] >= self.k]
        mask = sum(1 << q for q in glob)
        return [(mask, sum(((r >> (l2p[q] - self.k)) & 1) << q for q in glob)) for r in range(self.world)]

    def fingerprints(self, seed: int = 0) -> list:
        """Collective: every shard's fingerprint sum_i amp_i w(logical index of i) in its current (staged, moved) layout,
        gathered on every rank (qsim_fingerprint: evaluated on the device, two doubles per rank cross the links)."""
        self._flush_local()
        z = self.backend.fingerprint(self.n, self.rank << self.k, self.l2p, seed)
        return [complex(float(p[0]), float(p[1])) for p in self._gather([z.real, z.imag])]

    def _reference_fingerprints(self, cd: dict, selector_sets: list, seed: int) -> list:
        """Rank 0 only: the circuit on ONE device (the whole 2^n state next to the shard: n = 33 is 128 GiB of the 288),
        gate semantics and order of ref_dense.simulate (ref_dense.py:44-57) through the fused single-GPU path, then the
        fingerprint of every selector's index set.  Tests with a CPU backend replace this hook."""
        from quantum_simulations_amd.runner.engine import SingleGpuEngine
        if hasattr(self.backend, "release_buffers"):
            self.backend.release_buffers()
        one = SingleGpuEngine(self.n, device=self.backend.device, mode=self.mode)
        try:
            one.init_zero_state()
            one.execute(one.plan(cd))
            # (the one-GPU engine holds its state in a layout of its own choice: undone by the fingerprint itself)
            return [[one.state.fingerprint(self.n, 0, one.l2p, seed, m, v) for m, v in sel] for sel in selector_sets]
        finally:
            one.close()

    def check_against_single_device(self, cd: dict, runs: list, seed: int = 20260504) -> list:
        """Collective.  runs = [(fingerprints, selectors), ...] taken after executions of `cd` on the partition (one per
        layout / staging variant); returns per run max_r |shard fingerprint r - the same index set of a one-device run|.
        The one-device run happens once, on rank 0; the other ranks wait in the broadcast."""
        want = [None]
        if self.rank == 0:
            want = [self._reference_fingerprints(cd, [sel for _, sel in runs], seed)]
        self.dist.broadcast_object_list(want, src=0)
        return [max(abs(g - w) for g, w in zip(got, ref)) for (got, _), ref in zip(runs, want[0])]

    # ---- BASELINE configs 4 and 5 on this engine (bench.py at N > 1, tools/run_config.py) ----------------
    def _timed_circuit(self, cd: dict):
        """(seconds of ONE execution from |0..0>, steps of the plan); `last_plan_seconds` = the host time of the plan made for
        it -- start layouts, stage boundaries and tile passes -- which a one-shot run pays in front of the execution
        (it can exceed a GHZ's execution; the records carry both)."""
        self.init_zero_state()
        self.reset_comm_stats()
        self.barrier()
        t0 = time.perf_counter()
        plan = self.plan(cd)
        self.last_plan_seconds = self.max_over_ranks(time.perf_counter() - t0)
        self.barrier()
        t0 = time.perf_counter()
        self.execute(plan)
        self.barrier()
        dt = self.max_over_ranks(time.perf_counter() - t0)
        return dt, len(plan.executions[0])

    def run_baseline_configs(self, gen, check_amplitudes: bool = True) -> dict:
        """Config 5: n-qubit GHZ and GHZ+QFT, EVERY amplitude against the closed forms of SURVEY 8c on the
        devices (max-abs-error over all shards, staged layout included).  Config 4: the seeded Clifford+T
        circuit (depth 60) with and without staging: gate-applications/s, bytes over xGMI, exchange time -- and, like
        the random 1q+CX circuit of the timed region ("checked against a 1-GPU run"), its amplitudes
        against a one-GPU run of the same circuit through layout-aware per-shard fingerprints."""
        n = self.n
        out = {"config5": [], "config4": None}
        for kind, cd in (("ghz", gen.generate_ghz_circuit(n)), ("ghz_qft", gen.generate_ghz_qft(n))):
            dt, steps = self._timed_circuit(cd)
            err = self.closed_form_error(kind)
            err_host = self.closed_form_sample_error(kind)
            out["config5"].append({"circuit": kind, "n_qubits": n, "n_gpus": self.world, "gates": len(cd["gates"]), "layout": self.layout_info,
                                   "seconds": round(dt, 4), "gate_apps_per_s": round(len(cd["gates"]) / dt, 1),
                                   "plan_seconds": round(self.last_plan_seconds, 4),
                                   "gate_apps_per_s_incl_planning": round(len(cd["gates"]) / (dt + self.last_plan_seconds), 1),
                                   "steps": steps, "max_abs_err_vs_closed_form": err, "max_abs_err_sampled_host_check": err_host,
                                   "pass_1e-10": bool(err < 1e-10 and err_host < 1e-10),
                                   "norm2": self.norm2(), "xgmi": self.comm_stats()})
        seed = 20260504
        saved = self.staging
        for key, cd, variants in (("config4", gen.random_clifford_t_circuit(n, depth=60), (("staged", True), ("unstaged", False))),
                                  ("random_1q_cx", gen.random_1q_cx_circuit(n, depth=40), (("staged", True),))):
            rec = {"n_qubits": n, "n_gpus": self.world, "gates": len(cd["gates"]), "local_qubits": self.k}
            runs = []
            for label, staging in variants:
                self.staging = staging
                dt, steps = self._timed_circuit(cd)
                stats = self.comm_stats()
                ms = stats.get("exchange_ms_max_over_ranks")
                rec[label] = {"seconds": round(dt, 4), "gate_apps_per_s": round(len(cd["gates"]) / dt, 1), "steps": steps,
                              "plan_seconds": round(self.last_plan_seconds, 4),
                              "gate_apps_per_s_incl_planning": round(len(cd["gates"]) / (dt + self.last_plan_seconds), 1),
                              "hbm_passes": self.last_passes, "norm2": self.norm2(), "xgmi": stats,
                              # device-side exchange time (stream events, max over ranks; RCCL runs
                              # only) over the run's wall time -- pieces overlap compute, so this is an upper bound of
                              # what the links cost
                              "exchange_time_share": (round(ms * 1e-3 / dt, 4) if ms is not None else None),
                              "layout": self.layout_info}
                runs.append((self.fingerprints(seed), self.shard_selectors()))
            self.staging = saved
            if check_amplitudes:
                # EVERY amplitude of the partitioned result enters its shard's fingerprint; the same index sets of a one-GPU
                # run of the same circuit must give the same sums (north star: "matching reference amplitudes to 1e-10")
                diffs = self.check_against_single_device(cd, runs, seed)
                for (label, _), d in zip(variants, diffs):
                    rec[label]["fingerprint_max_abs_diff_vs_single_gpu"] = d
                    rec[label]["pass_1e-10"] = bool(d < 1e-10)
            out[key] = rec
        return out

    def measure_relayouts(self, reps: int = 2) -> list:
        """Collective.  What an all-to-all over m rank bits costs on THIS machine, m = 1 .. p, measured on the idle shard
        (whatever state it holds: every re-layout is made twice, there and back, so the state and the layout are the same
        afterwards): local bits k-1, k-2, ... trade places with rank bits 0, 1, ...  With nothing queued around it a
        re-layout is a pack pass, the exchange (piece by piece, all peers at once) and an unpack pass; reported per m:
        host-clock milliseconds (max over ranks) of the whole thing, device-event milliseconds of the exchange alone (RCCL
        runs: stream events from the first post to the last arrival; max over ranks), bytes per rank and the rate they
        give.  Replaces the modelled RELAYOUT_PASSES once a multi-GPU node has run it (bench.py prints
        `relayout_in_pass_units`)."""
        out = []
        shard_bytes = 16 << self.k
        for m in range(1, self.p + 1):
            pairs = [[self.k - 1 - i, self.k + i] for i in range(m)]
            if self.k - m < 3:
                break
            wall, events = [], []
            for _ in range(2 * max(1, reps)):
                self._flush_local()
                self.barrier()
                self.reset_comm_stats()
                t0 = time.perf_counter()
                self.relayout(pairs)
                self._flush_local()
                self.barrier()
                wall.append(self.max_over_ranks(time.perf_counter() - t0) * 1e3)
                events.append(self.comm_stats().get("exchange_ms_max_over_ranks"))
            sent = shard_bytes - (shard_bytes >> m)
            ev = [e for e in events if e]
            best_ev = min(ev) if ev else None
            out.append({"m": m, "local_bits": [pr[0] for pr in pairs], "bytes_sent_per_rank": sent, "pieces": self._relayout_pieces(self.k - m),
                        "wall_ms_pack_exchange_unpack": round(min(wall), 3), "exchange_event_ms": None if best_ev is None else round(best_ev, 3),
                        "exchange_GBps_per_rank": None if best_ev is None else round(sent / (best_ev * 1e-3) / 1e9, 1),
                        "wall_GBps_per_rank": round(sent / (min(wall) * 1e-3) / 1e9, 1), "repeats": 2 * max(1, reps)})
        self.reset_comm_stats()
        return out

    def comm_stats(self) -> dict:
        """Collective (every rank calls it): bytes and exchanges of this rank, device-side exchange time of this rank
        and the maximum over all ranks (RCCL runs only: stream events around every exchange)."""
        ms = ms_max = None
        if self._comm_events:
            self.backend.sync()
            ms = float(sum(a.elapsed_time(b) for a, b in self._comm_events))
        if not self.dry and self.dist.is_initialized() and self.dist.get_backend() == "nccl":
            ms_max = self.max_over_ranks(ms or 0.0)
        return {"bytes_sent_per_rank": self.xgmi_bytes_sent, "exchanges": self.exchanges,
                "exchange_ms_rank0": ms, "exchange_ms_max_over_ranks": ms_max}

    def reset_comm_stats(self) -> None:
        self.xgmi_bytes_sent, self.exchanges, self._comm_events, self.relayout_log = 0, 0, [], []

    def profile_begin(self) -> None:
        if hasattr(self.backend, "profile_begin"):
            self.backend.profile_begin()

    def profile_end(self):
        return self.backend.profile_end() if hasattr(self.backend, "profile_end") else []
