"""Plans of the multi-GPU engine (runner/distributed.py): the step lists of successive executions and the layout a fresh
state starts from.  Host work only.  |0..0> is the same state under every assignment of qubits to index bits, so the first
plan after `init_zero_state` may start from any -- which qubits are global first, which three sit on the line bits (they
belong to every tile) -- and the staged schedule that follows differs in re-layouts and HBM passes.  Staging method
"tiles": `choose_initial_layout_tiles`, a few assignments priced by the partition planner itself, the same on every rank
(deterministic, no collective).  Other methods: `choose_initial_layout`, LAYOUT_CANDIDATES random assignments each
executed on a planning twin of the engine (`_candidate_cost`), one all-reduce (the slowest rank decides).
"""
from __future__ import annotations

import time

import numpy as np

from quantum_simulations_amd.circuit.fusion import batch_levels
from quantum_simulations_amd.circuit.io import levelize, validate_circuit_dict
from quantum_simulations_amd.circuit.staging import atlas_stages
from quantum_simulations_amd.kernel import gates as gate_table
from quantum_simulations_amd.runner.shard_backends import PlanningBackend


class Plan:
    """Step lists for successive executions (the staging layout carries over between them).  `start_mappings[i]` is the planned
    layout execution i starts from; `execute` refuses a plan whose next execution was planned for another layout than the engine's."""

    def __init__(self, executions: list, mappings: list, start_mappings: list):
        self.executions, self.mappings, self.start_mappings, self.cursor = executions, mappings, start_mappings, 0


class PlanningMixin:
    """`plan` and what it needs, for `DistributedEngine` (which supplies the layout state, `execute` and `_reduce`)."""

    def _tiles_method(self) -> bool:
        """Staging method "tiles" applies: shards large enough for tile passes (the planner is the library's pass builder)."""
        return bool(self.staging and self.staging_method == "tiles" and 8 <= self.k <= 35 and self.n <= 63)

    def _fused_ops(self, cd: dict, l2p: list) -> list:
        """The circuit as an op list on the index bits of layout `l2p`, runs of 1q gates fused (fusion.py:41-81)."""
        from quantum_simulations_amd.circuit.fusion import fuse_1q_ops
        return fuse_1q_ops([([l2p[q] for q in g["qubits"]], gate_table.gate_matrix(g["gate"], g["params"])) for g in cd["gates"]])

    def _packed_ops(self, cd: dict):
        """`_fused_ops` in logical labels, packed once per circuit for the partition planner (relabelled per layout)."""
        from quantum_simulations_amd.runner.partition_plan import PackedOps
        key = id(cd)
        if getattr(self, "_packed_key", None) != key:
            self._packed, self._packed_key, self._packed_cd = PackedOps(self._fused_ops(cd, list(range(self.n))), self.n), key, cd
        return self._packed

    def _steps_from(self, cd: dict, l2p: list[int]):
        """Plan `cd` for a state whose logical qubit q currently sits at physical bit l2p[q]."""
        gates = [{"qubits": [l2p[q] for q in g["qubits"]], "gate": g["gate"], "params": g["params"]} for g in cd["gates"]]
        relabeled = {"number_of_qubits": self.n, "gates": gates}
        if self._tiles_method():
            # stage boundaries and tile passes planned together (runner/partition_plan.py)
            from quantum_simulations_amd.runner.partition_plan import MIN_OPS_CHOICES, plan_partition, plan_partition_best
            ops = self._packed_ops(cd).relabeled(l2p)
            if self.tiles_min_ops:
                res = plan_partition(ops, self.n, self.k, min_ops=self.tiles_min_ops, relayout_cost=self.RELAYOUT_PASSES)
            else:
                # (plans that run a few times search less: planning is host time the caller waits for)
                choices = MIN_OPS_CHOICES if self._plan_effort_high else (16, 24)
                res = plan_partition_best(ops, self.n, self.k, choices=choices, relayout_cost=self.RELAYOUT_PASSES, threads=self.plan_threads)
            self.last_partition_plan = res
            steps, moved = res["steps"], res["moved"]
        elif self.staging and self.k >= 2:   # (staging cannot hold a 2-qubit gate in fewer than 2 local qubits)
            # ("tiles" on shards too small for tile passes: the stage-by-stage method it replaces)
            steps, moved = atlas_stages(relabeled, self.k, method="belady" if self.staging_method == "tiles" else self.staging_method,
                                        strict_order=True)
        else:
            steps, moved = batch_levels(levelize(relabeled), self.k), list(range(self.n))
        return steps, [moved[l2p[q]] for q in range(self.n)]

    # ---- the initial layout ---------------------------------------------------------------------
    LAYOUT_CANDIDATES = 48
    # An all-to-all over m bits in units of one fused pass of the shard: (2^-m of the shard to each of 2^m - 1 peers, each
    # over its own xGMI link at 0.8 x 153 GB/s) / (the shard read and written once at 5 TB/s).  A MODEL -- no multi-GPU
    # node was available to measure it -- used only to weigh re-layouts against passes when two layouts differ in both.
    RELAYOUT_PASSES = {1: 10.4, 2: 5.2, 3: 2.6}

    def _candidate_cost(self, cd: dict, l2p: list, repeats: int = 1) -> tuple:
        """(cost in pass units per execution, HBM passes of the first execution, its re-layout sizes) of executing `cd`
        `repeats` times from |0..0> in the layout `l2p` ON THIS RANK: a shadow engine with a `PlanningBackend` runs the real
        schedule code -- staging, deferred local batches, rank-bit phases and conditional gates of this rank, fused
        re-layout ends -- without memory or arithmetic.  Later executions start from the layout the one before left behind;
        at most three are run, the mean of the second and third standing for all later ones."""
        sh = self._shadow
        if sh is None:
            sh = self._shadow = type(self)(self.n, self.world, self.rank, mode=self.mode, backend=PlanningBackend(self.k),
                                           staging=self.staging, staging_method=self.staging_method, init_process_group=False,
                                           relayout_pieces=self.relayout_pieces, min_piece_qubits=self.min_piece_qubits,
                                           fuse_relayout=self.fuse_relayout, layout="identity")
        sh.staging = self.staging
        sh.init_zero_state()
        sh._fresh = False
        sh.l2p_planned = list(l2p)
        run = max(1, min(repeats, 3))
        plan = sh.plan(cd, repeats=run)
        costs, first = [], None
        for _ in range(run):
            sh.backend.weight, sh.backend.passes, sh.relayout_log = 0.0, 0, []
            sh.execute(plan)
            costs.append(sh.backend.weight + sum(self.RELAYOUT_PASSES[m] for m in sh.relayout_log))
            first = first or (sh.last_passes, list(sh.relayout_log))
        later = float(np.mean(costs[1:])) if run > 1 else 0.0
        return (costs[0] + (max(1, repeats) - 1) * later) / max(1, repeats), first[0], first[1]

    def choose_initial_layout(self, cd: dict, n_candidates: int | None = None, seed: int = 20260504, repeats: int = 1) -> list:
        """l2p for a state that is still |0..0>: the identity or one of `n_candidates` random assignments, whichever gives
        the staged schedule of `cd` the lowest cost on the SLOWEST rank (`_candidate_cost` per rank, maximum over the ranks:
        they run different op lists; ties: the earlier candidate, the identity first).  COLLECTIVE."""
        n_candidates = self.LAYOUT_CANDIDATES if n_candidates is None else n_candidates
        rng = np.random.default_rng(seed)
        cands = [list(range(self.n))] + [[int(x) for x in rng.permutation(self.n)] for _ in range(n_candidates)]
        scored = [self._candidate_cost(cd, l2p, repeats) for l2p in cands]
        costs = [c for c, _, _ in scored]
        if self.dist.is_initialized() and self.world > 1:
            costs = self._reduce(costs, self.dist.ReduceOp.MAX)
        return self._keep_cheapest(cands, costs, scored, repeats)

    def _keep_cheapest(self, cands: list, costs, scored: list, repeats: int, **info) -> list:
        """The candidate of lowest cost (ties: the earlier one, the identity first); `layout_info`: chosen from what."""
        best = min(range(len(cands)), key=lambda i: (float(costs[i]), i))
        entry = lambda i: {"cost_max_over_ranks": round(float(costs[i]), 2), "passes_this_rank": scored[i][1],  # noqa: E731
                           "relayouts": scored[i][2]}
        self.layout_info = {"candidates": len(cands), "executions_planned_for": max(1, repeats), **info,
                            "identity": entry(0), "chosen": dict(entry(best), index=best)}
        return cands[best]

    LAYOUT_MIN_REPEATS = 8          # layout "auto": plans for fewer executions try 2 start layouts, not 17 (the search is host time)

    def choose_initial_layout_tiles(self, cd: dict, repeats: int = 1, n_candidates: int | None = None, seed: int = 20260504) -> list:
        """Staging method "tiles": l2p for a state that is still |0..0>.  Candidates: the identity, and assignments that put
        the p qubits whose FIRST use as a target comes last on the rank bits (Belady at time zero) with the other qubits
        in random order (which three sit on the line bits, members of every tile, moves the pass count), one in eight any
        assignment at all.  Each is priced by
        the partition planner itself -- passes + re-layouts in pass units of the first execution, and of a second one from
        the layout the first leaves behind when the plan will be repeated -- in parallel threads.  The planner names its
        tiles to the library, so what is priced is what every rank runs: no twin execution, no collective.  Deterministic."""
        from quantum_simulations_amd.runner.partition_plan import plan_partition, planning_pool
        t0 = time.perf_counter()
        n, k, p = self.n, self.k, self.p
        if n_candidates is None:
            n_candidates = 16 if self._plan_effort_high else 1     # (32 found nothing better on the seeded workloads)
        packed = self._packed_ops(cd)
        first = [1 << 60] * n
        for i, tg in enumerate(packed.targets):
            for q in tg:
                first[q] = min(first[q], i)
        far = sorted(range(n), key=lambda q: (-first[q], -q))[:p]
        rng = np.random.default_rng(seed)
        cands = [list(range(n))]
        for c in range(n_candidates):
            if c and c % 8 == 7:                      # (one in eight: any assignment at all)
                cands.append([int(x) for x in rng.permutation(n)])
                continue
            rest = [int(q) for q in (rng.permutation(n) if c else np.arange(n)) if q not in far]
            l2p = [0] * n
            for i, q in enumerate(rest):
                l2p[q] = i
            for i, q in enumerate(sorted(far)):
                l2p[q] = k + i
            cands.append(l2p)

        def price(l2p):
            costs, first_exec = [], None
            for _ in range(2 if repeats > 1 else 1):
                r = plan_partition(packed.relabeled(l2p), n, k, min_ops=self.tiles_min_ops or 24, relayout_cost=self.RELAYOUT_PASSES)
                costs.append(r["cost"])
                first_exec = first_exec or (r["passes"], r["relayouts"])
                l2p = [r["moved"][l2p[q]] for q in range(n)]
            later = costs[-1]
            return (costs[0] + (max(1, repeats) - 1) * later) / max(1, repeats), first_exec[0], first_exec[1]
        scored = list(planning_pool(self.plan_threads).map(price, cands)) if self.plan_threads > 1 else [price(c) for c in cands]
        best = self._keep_cheapest(cands, [c for c, _, _ in scored], scored, repeats, method="tiles")
        self.layout_info["search_seconds"] = round(time.perf_counter() - t0, 3)
        return best

    def plan(self, circuit_dict: dict, repeats: int = 1, effort: str | None = None) -> Plan:
        """Step lists for `repeats` successive executions from the engine's current layout.  Every rank must call it: the
        first plan of a freshly initialised state may search the start layout.  With staging method "tiles" each rank then
        computes the same choice on its own (deterministic, no collective); with the other methods the search is
        COLLECTIVE (`choose_initial_layout`: one all-reduce, the slowest rank's cost decides).  Host-only otherwise."""
        cd = validate_circuit_dict(circuit_dict)
        if cd["number_of_qubits"] != self.n:
            raise ValueError(f"circuit has {cd['number_of_qubits']} qubits, engine has {self.n}")
        # effort: "high" = the full search of start layouts and thin-pass thresholds (seconds of host time: worth it for a
        # plan that runs many times), "low" = two start layouts, two thresholds; None: by `repeats`
        self._plan_effort_high = (effort == "high") if effort else (repeats >= self.LAYOUT_MIN_REPEATS or self.layout == "search")
        was_fresh = self._fresh and self.layout != "identity"
        if self._fresh:
            # (once per initialised state: a second plan made before the first one runs keeps this layout, so both stay valid)
            self._fresh = False
            if self.world > 1 and self.k >= 2 and (self.layout == "search" or (self.layout == "auto" and self.k >= 20)):
                if self._tiles_method():
                    self.l2p_planned = self.choose_initial_layout_tiles(cd, repeats=max(1, repeats))
                else:
                    t0 = time.perf_counter()
                    self.l2p_planned = self.choose_initial_layout(cd, repeats=max(1, repeats))
                    self.layout_info["search_seconds"] = round(time.perf_counter() - t0, 3)
        executions, mappings, starts = [], [], []
        l2p = list(self.l2p_planned)
        for _ in range(max(1, repeats)):
            starts.append(list(l2p))
            steps, l2p = self._steps_from(cd, l2p)
            executions.append(steps)
            mappings.append(list(l2p))
        if was_fresh and self.place_slots and self._tiles_method() and self.k >= self.place_slots_min_k:
            # |0..0> looks the same under every assignment of qubits to index bits: the local slots of the whole chain of
            # executions are put on the index bits whose tiles have the best DRAM pattern (partition_plan.place_slots)
            from quantum_simulations_amd.runner.partition_plan import place_slots
            t0 = time.perf_counter()
            sigma, before, after = place_slots(executions, self.k)
            if sigma is not None:
                mp = lambda b: sigma.get(b, b)                           # noqa: E731
                starts = [[mp(b) for b in m] for m in starts]
                mappings = [[mp(b) for b in m] for m in mappings]
                self.l2p_planned = list(starts[0])
                self.layout_info = dict(self.layout_info or {}, slot_placement={
                    "tile_model_ms_per_plan": [round(before, 2), round(after, 2)], "seconds": round(time.perf_counter() - t0, 3)})
        return Plan(executions, mappings, starts)

    def passes_per_step(self, plan: Plan) -> int:
        """HBM passes of the last executed circuit on this rank: fused tile launches of the local steps, + 1 for every
        pack / unpack of a re-layout that could not ride in a neighbouring fused pass (2 per re-layout with
        fuse_relayout=False); before any execution, the op count of the plan."""
        if self.last_passes:
            return self.last_passes
        return sum(len(s["local_ops"]) + len(s["nonlocal_ops"]) for s in plan.executions[0])

