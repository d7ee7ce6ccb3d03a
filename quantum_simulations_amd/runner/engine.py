"""Execution engines: one HBM-resident state (single GPU) or one shard per rank (multi-GPU).

This is the collapsed form of the reference's runner layer (wenbo_engine/runner/
single_node.py:141-321): with the state resident in HBM a step is "launch kernels /
exchange / launch kernels" -- no chunk files, no double-buffer directories.

`make_engine(n, world, rank, local_rank)` returns an object with
    init_zero_state(), plan(circuit_dict) -> plan, execute(plan), barrier(), norm2(),
    state_vector() (logical order, gathered on every rank), close()
used by bench.py, the v3-style Driver and the tests.
The calls on the state (expectation, evolve, qaoa, gradient, ...) are `state_calls.StateCalls`, the layout search is
`runner/layout_search.py` (its names are imported here), bench.py's ceilings and gate sweep are `runner/measure.py`.
"""
from __future__ import annotations

from contextlib import contextmanager

import numpy as np

from quantum_simulations_amd.circuit.fusion import batch_levels
from quantum_simulations_amd.circuit.io import levelize, validate_circuit_dict
from quantum_simulations_amd.kernel import gates as gate_table, planner
from quantum_simulations_amd.kernel.device import DeviceChunk
from quantum_simulations_amd.runner import measure
from quantum_simulations_amd.runner.layout_search import (_count_passes, choose_plan_layout, layout_swaps,  # noqa: F401
                                                          pass_memory_us, priced_variant)
from quantum_simulations_amd.state_calls import StateCalls


def gate_ops(cd: dict) -> list:
    """Validated circuit -> [(qubits, U)] in list order (no levelling, no fusion)."""
    return [(g["qubits"], gate_table.gate_matrix(g["gate"], g["params"])) for g in cd["gates"]]


class GpuPlan(list):
    """A single-GPU plan: the list of batches ((nq, qubits, mats) packed for ONE C call each, in PHYSICAL index bits) plus
    `tiles` (per batch the high tile bits of its fused passes as uint64 masks, or None: let the library search) and `l2p`
    (the qubit layout the batches were written for: logical qubit q on index bit l2p[q]; None = identity)."""
    tiles: list
    placed: list | None = None           # per batch the placement of its ops over the named passes (int32 per op: `planner.balance`), or None
    l2p: list | None = None
    model_ms: tuple | None = None        # (identity, chosen) totals of the tile-cost model over the passes, when a layout was chosen
    cycle = None                         # a cyclic plan (`device.Cycle`): `execute` defers the tail of every execution to the next; the
                                         # list itself then holds the steady op list, for callers that look at it


class SingleGpuEngine(StateCalls):
    """The whole 2^n state on one MI355X (n <= 33 fits 288 GB).

    layout = "auto" (fused mode, states of >= 26 qubits, plans made for >= 8 executions) / "search" (always): `plan`
    decides which index bit every logical qubit lives on --
      * the three qubits on the LINE bits 0..2 belong to every tile, so which three they are changes how many passes a
        plan needs (16-18 for the 28-qubit bench circuit under the searching pass builder, `qsim_plan_search`; the
        greedy builder of one-shot calls needs 17-20): a few dozen random triples are searched on the host in parallel
        and the cheapest kept;
      * the other qubits are placed so that the passes' tiles fall on index-bit sets with a good DRAM pattern
        (runner/tile_layout.py: a cost model fitted to measured passes, annealed by `qsim_choose_layout`) --
    and hands the SAME passes to the library on the new bits (`qsim_apply_ops_tiled`).  The state is then held in that
    layout -- the reference's `log_to_phys` notion (staging.py:587-658) -- and `state_vector()` / `logical_index()` undo
    it.  A few seconds of host work per plan, outside every timed region: worth it for plans that run many times.
    layout = "identity": index bit = qubit, no search."""

    world = 1
    rank = 0
    LAYOUT_MIN_QUBITS = 26
    LAYOUT_MIN_REPEATS = 8         # layout = "auto": plans for fewer executions are not worth a second of search
    LAYOUT_CANDIDATES = 63         # random line-qubit triples (next to the identity) searched in one library call (qsim_plan_search_triples)
    LAYOUT_BEAM = 0                # beam width of the pass search (0: the library's default)
    LAYOUT_FINALISTS = 8           # minimum-pass layouts timed on the device (tune_on_device, |0..0> state only)
    CYCLES = True                  # plans of one op list made for LAYOUT_MIN_REPEATS executions or more may be cyclic (`planner.search_cycle`);
                                   # False: every execution is planned as if it stood alone (A/B runs)
    ENGINE_PRICING = True          # plans made for many executions price the gate engine (runner/engine_cost.py): rule (d) of the
                                   # op rewrite, and ops that need no tile leave the passes whose records cost more than their memory time

    def __init__(self, n_qubits: int, device: int = 0, mode: str = "fused", layout: str = "auto", tune_on_device: bool = False):
        if layout not in ("auto", "search", "identity"):
            raise ValueError("layout must be 'auto', 'search' or 'identity'")
        self.n = n_qubits
        self.mode = mode
        self.layout_mode = layout
        self.tune_on_device = bool(tune_on_device)   # plan(): time the minimum-pass layouts on the device when the state is |0..0>
        self.state = DeviceChunk.empty(n_qubits, device)
        self.l2p: list | None = None        # layout of the state right now (None = identity)
        self._zero = False                  # the state is |0..0>: the same vector in every layout
        self._work: DeviceChunk | None = None   # a second chunk of the state's size (H|psi>, lambda): allocated on first use

    # ---- state ---------------------------------------------------------------------
    def init_zero_state(self) -> None:
        self.state.init_zero(True)
        self.l2p, self._zero = None, True

    def init_random_state(self, seed: int) -> None:
        self.state.init_random(seed)
        self.l2p, self._zero = None, False

    def norm2(self) -> float:
        return self.state.norm2()

    def state_vector(self) -> np.ndarray:
        """The state in LOGICAL qubit order (the layout undone on the host: small n)."""
        psi = self.state.download()
        if self.l2p is None:
            return psi
        from quantum_simulations_amd.circuit.staging import permute_state
        return permute_state(psi, self.l2p)

    # ---- the state calls (state_calls.StateCalls) run on `state` through `l2p`; the engine's two hooks ------------------------
    @contextmanager
    def _second_chunk(self):
        """The engine's own second chunk: allocated on first use, kept, closed in `close()`."""
        if self._work is None:
            self._work = self._new_chunk()
        yield self._work

    def _state_written(self) -> None:
        self._zero = False

    def logical_index(self, offset: int, count: int) -> np.ndarray:
        """Logical amplitude indices of the physical range [offset, offset + count) of the state in its current layout."""
        x = offset + np.arange(count, dtype=np.int64)
        if self.l2p is None:
            return x
        y = np.zeros_like(x)
        for q, p in enumerate(self.l2p):
            y |= ((x >> p) & 1) << q
        return y

    # ---- planning / execution --------------------------------------------------------
    def plan(self, circuit_dict: dict, repeats: int = 1) -> GpuPlan:
        """Plan = list of batches, each handed to ONE C call (the same plan serves every repeat: the layout of a
        single-GPU run is chosen once per plan and never changes)."""
        cd = validate_circuit_dict(circuit_dict)
        if cd["number_of_qubits"] != self.n:
            raise ValueError(f"circuit has {cd['number_of_qubits']} qubits, engine has {self.n}")
        from quantum_simulations_amd.kernel.device import pack_ops
        if self.mode == "per-gate":
            plan = GpuPlan([pack_ops(gate_ops(cd))])
            plan.tiles = [None]
            return plan
        return self.plan_batches([p["local_ops"] for p in batch_levels(levelize(cd), self.n)], repeats)

    def plan_batches(self, batches, repeats: int = 1) -> GpuPlan:
        """`plan` for op lists [(qubits, U), ...] (one C call each) instead of a circuit dict: what a caller with gates
        outside the circuit contract (a dense 4x4, collapse factors) plans with.  Fused mode."""
        from quantum_simulations_amd.kernel.device import pack_ops
        search = self.layout_mode == "search" or (self.layout_mode == "auto" and repeats >= self.LAYOUT_MIN_REPEATS)
        if not search or self.n < self.LAYOUT_MIN_QUBITS:
            plan = GpuPlan([pack_ops(ops) for ops in batches])
            plan.tiles = [None] * len(batches)
            return plan
        import time
        t0 = time.perf_counter()
        tune = self.tune_on_device and self._zero            # (timing runs overwrite the state: only |0..0> can be put back)
        plans = self.finalist_plans(batches, self.LAYOUT_FINALISTS if tune else 4, repeats)
        chosen = plans[0]
        if tune and len(plans) > 1:
            timed = self._time_on_device(plans)
            chosen = plans[int(np.argmin(timed))]
            chosen.layout_info["tuned_on_device_ms"] = [round(t, 3) for t in timed]
        chosen.layout_info["seconds"] = round(time.perf_counter() - t0, 3)
        return chosen

    def finalist_plans(self, batches, n_finalists: int, repeats: int = 1) -> list:
        """The plans of up to n_finalists minimum-pass layouts of the op lists `batches` (`choose_plan_layout` over the
        identity and LAYOUT_CANDIDATES random line-qubit triples), lowest modelled time first: what `plan_batches` chooses
        from -- the first, or the one the device runs fastest (tune_on_device).  One op list planned for `repeats` >=
        LAYOUT_MIN_REPEATS executions (and CYCLES): the cyclic plans found for it are finalists too, next to the plain ones."""
        from quantum_simulations_amd.kernel.device import Cycle, pack_ops
        cycle_repeats = repeats if self.CYCLES and len(batches) == 1 and repeats >= self.LAYOUT_MIN_REPEATS else 0
        # What the planner is given: the batches with their X / Y gates pushed into neighbouring gates and their H-framed
        # CNOTs turned into CZ (csrc/op_rewrite.h) -- the same amplitudes from fewer ops that need their target inside a
        # tile, hence fewer passes (16 -> 13 on the 28-qubit bench circuit).  `passes_identity` stays what it was:
        # the greedy identity-layout count of the circuit's own ops.
        own_batches, rewrite = batches, {"ops_in": 0, "ops_out": 0, "need_tile_in": 0, "need_tile_out": 0}
        from quantum_simulations_amd.runner import engine_cost
        costs = engine_cost.table() if self.ENGINE_PRICING else None
        batches = []
        for ops in own_batches:
            stats = {}
            batches.append(planner.rewrite_ops(self.n, ops, stats))
            for key in rewrite:
                rewrite[key] += stats[key]
        # ... and, priced (runner/engine_cost.py), the same lists with rule (d): diagonal 1q gates multiplied into dense ones
        # where the engine cost table prices the product's record lower.  The tiles are searched on the lists above -- ops
        # that need no tile fewer never cost a pass under the same tiles -- and every finalist keeps whichever list the
        # model prices lower under them (`priced_variant`).
        priced = None if costs is None else [planner.rewrite_ops(self.n, ops, None, costs) for ops in own_batches]
        own_identity = int(_count_passes(self.n, own_batches, np.arange(self.n, dtype=np.int32)[None, :], 1)[0])
        finalists = choose_plan_layout(self.n, batches, self.LAYOUT_CANDIDATES, n_finalists=n_finalists,
                                       all_finalists=True, beam=self.LAYOUT_BEAM, engine_costs=costs, priced_batches=priced,
                                       cycle_repeats=cycle_repeats)

        def build(l2p, masks, info):
            cyc = info.pop("cycle", None)
            if cyc is not None:                                 # (head, steady, tail: `planned` is the steady list)
                info.pop("planned", None)
                info.pop("placed", None)
                plan = GpuPlan([pack_ops(cyc["planned"][1])])
                plan.cycle = Cycle(self.n, *zip(cyc["planned"], cyc["tiles"], cyc["placed"]))
                plan.tiles, plan.placed = masks, [cyc["placed"][1]]
                plan.l2p = None if l2p == list(range(self.n)) else l2p
                plan.model_ms = info["model_ms"]
                plan.layout_info = dict(info, passes_identity=own_identity, rewrite=dict(rewrite), cycle_passes=dict(
                    zip(("head", "steady", "tail"), plan.cycle.passes), plain=cyc["plain_passes"]))
                return plan
            planned = info.pop("planned", None) or [[([l2p[q] for q in qs], U) for qs, U in ops] for ops in batches]
            plan = GpuPlan([pack_ops(ops) for ops in planned])
            plan.tiles = masks
            plan.placed = info.pop("placed", None)
            plan.l2p = None if l2p == list(range(self.n)) else l2p
            plan.model_ms = info["model_ms"]
            plan.layout_info = dict(info, passes_identity=own_identity, rewrite=dict(rewrite))
            return plan
        return [build(*f) for f in finalists]

    def _time_on_device(self, plans) -> list:
        """Milliseconds of every plan on the device.  The cost model cannot rank the minimum-pass layouts (measured: 3 %
        apart, uncorrelated with the model): the device can -- the better of two timed executions of each on the (zero)
        state, which is |0..0> again afterwards.  A cyclic plan is timed alike: after its first execution (the head) the
        timed ones run its steady passes -- `time_begin` / `time_end` do not run a deferred tail -- and `init_zero_state`
        drops the tail that is left."""
        timed = []
        for p in plans:
            self.init_zero_state()
            self.execute(p)
            ms = []
            for _ in range(2):
                self.state.time_begin()
                self.execute(p)
                ms.append(self.state.time_end())
            timed.append(min(ms))
        self.init_zero_state()
        return timed

    def _adopt_layout(self, l2p) -> None:
        """Bring the state into the layout a plan was written for."""
        if l2p == self.l2p or (l2p is None and self.l2p == list(range(self.n))):
            return
        if self._zero:                      # |0..0> looks the same in every layout
            self.l2p = l2p
            return
        # a non-trivial state: move the qubits with SWAP gates (fused passes; rare -- a new plan on a used state)
        SW = gate_table.SWAP()
        swaps = [([a, b], SW) for a, b in layout_swaps(self.l2p, l2p, self.n)]
        if swaps:
            self.state.apply_ops(swaps)
        self.l2p = l2p

    def execute(self, plan) -> None:
        self._adopt_layout(getattr(plan, "l2p", None))
        self._zero = False
        self.last_passes = 0
        if getattr(plan, "cycle", None) is not None and self.mode != "per-gate":
            self.last_passes = self.state.apply_cycle(plan.cycle)
            return
        tiles = getattr(plan, "tiles", None) or [None] * len(plan)
        placed = getattr(plan, "placed", None) or [None] * len(plan)
        for ops, masks, place in zip(plan, tiles, placed):
            if masks is not None and place is not None and self.mode != "per-gate":
                self.last_passes += self.state.apply_ops_placed(ops, masks, place)
            elif masks is not None and self.mode != "per-gate":
                self.last_passes += self.state.apply_ops_tiled(ops, masks)
            else:
                self.last_passes += self.state.apply_ops(ops, fused=self.mode != "per-gate")

    def passes_per_step(self, plan: list) -> int:
        """HBM round trips of the last executed step (fused tile launches or single gates)."""
        return getattr(self, "last_passes", sum(len(ops[0]) for ops in plan))

    # ---- synchronisation / measurement --------------------------------------------------
    def barrier(self) -> None:
        self.state.sync()

    def max_over_ranks(self, value: float) -> float:
        return value

    def profile_begin(self) -> None:
        self.state.profile_begin()

    def profile_end(self) -> list[dict]:
        return self.state.profile_end()

    def sweep_gates(self, n: int, reps: int = 5) -> dict:
        """`measure.sweep_gates` on the engine's state when n is its size (which it overwrites), else on a chunk of its own."""
        if n == self.n:
            self.l2p, self._zero = None, False
        return measure.sweep_gates(self.state, n, reps)

    def copy_ceiling(self, reps: int = 7) -> dict:
        return measure.copy_ceiling(self.state, reps)

    def stream_ceiling(self, reps: int = 5) -> dict:
        return measure.stream_ceiling(self.state, reps)

    def prefix_parity(self, circuit_dict: dict, n_gates: int, expected: np.ndarray) -> float:
        """max |amp - expected| after the first n_gates gates from |0..0> (checker hook for bench.py's CPU leg; runs
        outside every timed region) -- through the SAME path as the timed steps: planned by `plan` (layout search and named
        tiles included, when the engine uses them), executed, compared through the layout."""
        cd = validate_circuit_dict(circuit_dict)
        prefix = {"number_of_qubits": self.n, "gates": cd["gates"][:n_gates]}
        self.init_zero_state()
        tune, self.tune_on_device = self.tune_on_device, False          # (no timing runs for a check)
        try:
            plan = self.plan(prefix, repeats=self.LAYOUT_MIN_REPEATS)
        finally:
            self.tune_on_device = tune
        self.execute(plan)
        worst = 0.0
        step = 1 << 24
        for off in range(0, 1 << self.n, step):
            cnt = min(step, (1 << self.n) - off)
            got = self.state.download(off, cnt)
            want = expected[off:off + cnt] if self.l2p is None else expected[self.logical_index(off, cnt)]
            worst = max(worst, float(np.max(np.abs(got - want))))
        self.last_parity_layout = None if self.l2p is None else list(self.l2p)
        return worst

    def close(self) -> None:
        if self._work is not None:
            self._work.close()
            self._work = None
        self.state.close()


def _planned_tile_masks(n: int, ops) -> np.ndarray:
    """The earlier name of `planner.tile_masks(planner.plan_ops(n, ops))` (no masks for fewer than two ops), kept because
    callers outside the package import it; new code uses the planner module."""
    return planner.tile_masks(planner.plan_ops(n, ops)) if len(ops) >= 2 else np.zeros(0, dtype=np.uint64)


def make_engine(n_qubits: int, world: int = 1, rank: int = 0, local_rank: int = 0,
                mode: str = "fused", **kw):
    if world == 1:                      # (rehearsal / exchange only mean something with more than one rank)
        return SingleGpuEngine(n_qubits, device=local_rank, mode=mode, layout=kw.get("layout", "auto"),
                               tune_on_device=kw.get("tune_on_device", False))
    from quantum_simulations_amd.runner.distributed import DistributedEngine
    return DistributedEngine(n_qubits, world, rank, local_rank, mode=mode, **kw)
