"""Execution engines: one HBM-resident state (single GPU) or one shard per rank (multi-GPU).

This is the collapsed form of the reference's runner layer (wenbo_engine/runner/
single_node.py:141-321): with the state resident in HBM a step is "launch kernels /
exchange / launch kernels" -- no chunk files, no double-buffer directories.

`make_engine(n, world, rank, local_rank)` returns an object with
    init_zero_state(), plan(circuit_dict) -> plan, execute(plan), barrier(), norm2(),
    state_vector() (logical order, gathered on every rank), close()
used by bench.py, the v3-style Driver and the tests.
"""
from __future__ import annotations

import numpy as np

from quantum_simulations_amd import diagonal, evolution, hamiltonian, krylov, readout
from quantum_simulations_amd.circuit.fusion import batch_levels
from quantum_simulations_amd.circuit.io import levelize, validate_circuit_dict
from quantum_simulations_amd.kernel import gates as gate_table, planner
from quantum_simulations_amd.kernel.device import DeviceChunk


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


class SingleGpuEngine:
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
    LAYOUT_CANDIDATES = 31         # random line-qubit triples (next to the identity) whose plans are searched
    LAYOUT_BEAM = 0                # beam width of the pass search (0: the library's default)
    LAYOUT_FINALISTS = 8           # minimum-pass layouts timed on the device (tune_on_device, |0..0> state only)
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

    def expectation(self, obs) -> float:
        """<psi|H|psi> (unnormalised) of a Pauli sum over LOGICAL qubits (observable.PauliSum or what it accepts),
        evaluated on the device through the current layout; the state does not move."""
        return readout.expectation(self.state, self.l2p, obs)

    def apply_pauli_rotations(self, rotations) -> int:
        """psi := exp(-i theta P) psi for every entry of `rotations`, first entry first, on the device through the
        current layout (the state does not move).  No factor 1/2 on theta.  `rotations`: the (x, z, theta) arrays of
        `evolution.trotter_rotations` over LOGICAL qubits, or a list of (pauli, theta) pairs / (x, z, theta) triples
        (`evolution.rotation`).  Returns the HBM passes made."""
        passes = evolution.apply_rotations(self.state, self.l2p, rotations)
        self._zero = False
        return passes

    def evolve(self, obs, t, steps: int = 1, order: int = 1, fuse_diagonal: bool = False) -> int:
        """exp(-i t H) psi by a product formula (`evolution.trotter_rotations`: order 1 or the symmetric order 2,
        `steps` steps) of the Pauli sum H over LOGICAL qubits, applied on the device through the current layout; the
        state does not move.  `fuse_diagonal`: runs of Z-only rotations go through one diagonal phase pass each
        (`evolution.apply_rotations`).  Returns the HBM passes made."""
        passes = evolution.evolve(self.state, self.l2p, obs, t, steps, order, fuse_diagonal)
        self._zero = False
        return passes

    def apply_diagonal_phase(self, obs, gamma) -> int:
        """psi := exp(-i gamma D) psi for a diagonal Pauli sum D (Z and identity only) over LOGICAL qubits: ONE pass on
        the device whatever the number of terms, through the current layout; the state does not move.  No factor 1/2
        (`diagonal.apply_phase`).  Returns the HBM passes made."""
        passes = diagonal.apply_phase(self.state, self.l2p, obs, gamma)
        self._zero = False
        return passes

    def diagonal_moments(self, obs) -> tuple:
        """(<D>, <D^2> - <D>^2) of a diagonal Pauli sum over LOGICAL qubits in the normalised state, from one read-only
        pass on the device through the current layout (`diagonal.moments`)."""
        return diagonal.moments(self.state, self.l2p, obs)

    def qaoa(self, cost, gammas, betas) -> int:
        """QAOA layers on the current state: per layer exp(-i gamma_l C) for the diagonal cost C over LOGICAL qubits
        (one pass), then exp(-i beta_l X_q) on every qubit; no factor 1/2 (`diagonal.qaoa`).  The state does not move.
        Returns the HBM passes made."""
        passes = diagonal.qaoa(self.state, self.l2p, cost, gammas, betas)
        self._zero = False
        return passes

    def qaoa_gradient(self, cost, gammas, betas) -> tuple:
        """(E, dE/dgammas, dE/dbetas) of E = <psi|C|psi> with psi = the QAOA circuit of `qaoa` applied to the CURRENT
        state, by the adjoint method on the device (`diagonal.qaoa_gradient`: per layer one overlap with the n mixer
        strings, one diagonal overlap pass and the two inverse layers on two chunks); no factor 1/2, unnormalised.  The
        state is the same afterwards up to rounding and does not move; the engine's second chunk is overwritten."""
        out = diagonal.qaoa_gradient(self.state, self._work_chunk(), self.l2p, cost, gammas, betas)
        self._zero = False
        return out

    def _work_chunk(self) -> DeviceChunk:
        if self._work is None:
            self._work = DeviceChunk.empty(self.n, self.state.device)
        return self._work

    def apply_observable(self, obs, out: DeviceChunk | None = None, fuse_diagonal: bool = False) -> DeviceChunk:
        """H|psi> for a Pauli sum over LOGICAL qubits, written on the device into `out` (a chunk of the state's size
        on its device; default: the engine's own second chunk, allocated on first use and overwritten by `variance` and
        `gradient`) IN THE STATE'S CURRENT LAYOUT `self.l2p`; the state does not move.  Returns that chunk;
        `out.last_pauli_sum_passes` = the HBM passes made by the per-term path.  `fuse_diagonal`: the Z-only terms go
        through one diagonal pass more (`hamiltonian.apply`)."""
        out = self._work_chunk() if out is None else out
        hamiltonian.apply(out, self.state, self.l2p, obs, fuse_diagonal)
        return out

    def variance(self, obs, fuse_diagonal: bool = False) -> float:
        """<H^2> - <H>^2 (unnormalised: norm2(H psi) - <psi|H|psi>^2) of a Pauli sum over LOGICAL qubits, on the
        device; the engine's second chunk is overwritten.  `fuse_diagonal`: as in `apply_observable`."""
        return hamiltonian.variance(self.state, self._work_chunk(), self.l2p, obs, fuse_diagonal)

    def overlap_with(self, chunk: DeviceChunk, obs=None):
        """<chunk|psi> (obs None: a complex number), or <chunk|H|psi> = sum_t c_t <chunk|P_t|psi> for a Pauli sum over
        LOGICAL qubits, on the device; `chunk` holds a state of the same size in the state's current layout `self.l2p`
        (what `apply_observable` writes, or a copy of an earlier state).  Neither state moves."""
        if obs is None:
            return self.state.overlap(chunk)
        from quantum_simulations_amd.observable import as_pauli_sum
        obs = as_pauli_sum(obs, self.n)
        terms = hamiltonian.matrix_elements(self.state, chunk, self.l2p, obs)
        return complex(sum(float(c) * complex(v) for c, v in zip(obs.coeffs, terms)))

    def gradient(self, rotations, obs) -> tuple:
        """(E, dE/dtheta) of E = <psi(theta)|H|psi(theta)> with psi(theta) = the rotation list (every entry its own
        parameter, exp(-i theta P) without a factor 1/2; forms as in `apply_pauli_rotations`) applied to the CURRENT
        state, by the adjoint method on the device (`hamiltonian.adjoint_gradient`: one forward run, then one overlap
        and two single-rotation passes per parameter).  The state is the same afterwards up to rounding; the engine's
        second chunk is overwritten."""
        out = hamiltonian.adjoint_gradient(self.state, self._work_chunk(), self.l2p, rotations, obs)
        self._zero = False
        return out

    def _with_krylov_chunks(self, m: int, call):
        """call(work) with `m` chunks of the state's size that live for the call only (everything allocated so far is
        closed when an allocation fails); `variance`'s second chunk is not touched."""
        work = []
        try:
            for _ in range(max(int(m), 0)):
                work.append(DeviceChunk.empty(self.n, self.state.device))
            self._zero = False
            return call(work)
        finally:
            for c in work:
                c.close()

    def ground_state(self, obs, m: int = 16, tol: float = 1e-8, max_restarts: int = 50, fuse_diagonal: bool = False) -> tuple:
        """The lowest eigenpair of a Pauli sum over LOGICAL qubits by restarted Lanczos on the device
        (`krylov.ground_state`), started from the CURRENT state, which must overlap the ground state
        (`init_random_state` does) and is replaced by the normalised eigenvector estimate in the current layout.
        m + 1 chunks of the state's size are alive during the call: m work chunks are allocated for it and freed.
        Returns (energy, residual |H psi - E psi|, restarts, H applications).  `fuse_diagonal`: as in `apply_observable`,
        for every H application."""
        return self._with_krylov_chunks(m, lambda work: krylov.ground_state(self.state, work, self.l2p, obs, m, tol, max_restarts,
                                                                            fuse_diagonal=fuse_diagonal))

    def evolve_krylov(self, obs, t, m: int = 16, steps: int = 1, fuse_diagonal: bool = False) -> float:
        """psi := exp(-i t H) psi to Krylov accuracy (`krylov.evolve`: `steps` steps of m Lanczos vectors each) for a
        Pauli sum over LOGICAL qubits, on the device through the current layout; t = -i tau gives exp(-tau H) psi,
        unnormalised.  m work chunks are allocated for the call and freed.  Returns the a-posteriori error estimate.
        `fuse_diagonal`: as in `apply_observable`, for every H application."""
        return self._with_krylov_chunks(m, lambda work: krylov.evolve(self.state, work, self.l2p, obs, t, m, steps, fuse_diagonal))

    def reduced_density_matrix(self, qubits) -> np.ndarray:
        """Reduced density matrix (unnormalised, complex128 (2^r, 2^r)) of 1 to 6 LOGICAL qubits, bit j of a row or
        column index = qubit qubits[j], evaluated on the device through the current layout; the state does not move."""
        return readout.reduced_density_matrix(self.state, self.l2p, qubits)

    def sample(self, shots: int, seed: int = 0, qubits=None) -> np.ndarray:
        """`shots` samples of the register, drawn on the device through the current layout (the state does not move;
        `sampling.draw(shots, seed)` gives the uniforms): LOGICAL basis-state indices as uint64, or with `qubits` the
        marginal values (bit j = qubit qubits[j]).  `sampling.counts` turns them into {bitstring: count}."""
        return readout.sample(self.state, self.l2p, shots, seed, qubits)

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
        finalists = choose_plan_layout(self.n, batches, self.LAYOUT_CANDIDATES, n_finalists=self.LAYOUT_FINALISTS if tune else 4,
                                       all_finalists=True, beam=self.LAYOUT_BEAM, engine_costs=costs, priced_batches=priced)

        def build(l2p, masks, info):
            planned = info.pop("planned", None) or [[([l2p[q] for q in qs], U) for qs, U in ops] for ops in batches]
            plan = GpuPlan([pack_ops(ops) for ops in planned])
            plan.tiles = masks
            plan.placed = info.pop("placed", None)
            plan.l2p = None if l2p == list(range(self.n)) else l2p
            plan.model_ms = info["model_ms"]
            plan.layout_info = dict(info, passes_identity=own_identity, rewrite=dict(rewrite))
            return plan
        plans = [build(*f) for f in finalists]
        chosen = plans[0]
        if tune and len(plans) > 1:
            # the cost model cannot rank the minimum-pass layouts (measured: 3 % apart, uncorrelated with the model): the
            # device can -- two timed executions of each on the (zero) state, which is |0..0> again afterwards
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
            chosen = plans[int(np.argmin(timed))]
            chosen.layout_info["tuned_on_device_ms"] = [round(t, 3) for t in timed]
            self.init_zero_state()
        chosen.layout_info["seconds"] = round(time.perf_counter() - t0, 3)
        return chosen

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
        """BASELINE config 3: one gate per launch on an n-qubit random state, per-target HIP-event
        timing (median of `reps`), as fractions of the 8 TB/s HBM peak of SURVEY 8d's algorithmic bytes:
        H(q) 32 * 2^n for every q; secondary rows T(q), CNOT(q, q+1), CNOT(0, q) at 16 * 2^n."""
        dev = self.state if n == self.n else DeviceChunk.empty(n, self.state.device)
        dev.init_random(30)
        if dev is self.state:
            self.l2p, self._zero = None, False
        H, T, CX = gate_table.H(), gate_table.T(), gate_table.CNOT()
        N = 1 << n

        def timed(fn) -> float:
            fn()
            dev.sync()
            ts = []
            for _ in range(reps):
                dev.time_begin()
                fn()
                ts.append(dev.time_end())
            return float(np.median(ts))

        def moved_bytes(fn) -> float:
            """bytes the launch(es) of one gate really move (the library's own per-launch accounting: 32 B per amplitude
            a launch touches -- all of them when a diagonal / control bit lies inside a 128-B line)"""
            dev.profile_begin()
            fn()
            return float(sum(e["hbm_bytes"] for e in dev.profile_end()))

        def row(label, targets, fn, nbytes, note=None) -> dict:
            ms = [timed(lambda q=q: fn(q)) for q in targets]
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
            ms = [timed(lambda qs=qs: dev.apply_fused_k(qs, M)) for qs in sets]
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
        if dev is not self.state:
            dev.close()
        return {"n_qubits": n, "reps": reps, "rows": rows, "dense_blocks": dense, "norm2_after": norm2}

    def copy_ceiling(self, reps: int = 7) -> dict:
        """Same-run device-to-device copy of a buffer of the state's size (qsim_copy: streaming loads and
        stores, 32 B moved per amplitude): the practical HBM ceiling next to the nominal 8 TB/s."""
        other = DeviceChunk.empty(self.n, self.state.device)
        other.copy_from(self.state)
        other.sync()
        ts = []
        for _ in range(reps):
            other.time_begin()
            other.copy_from(self.state)
            ts.append(other.time_end())
        other.close()
        ms = float(np.median(ts))
        gbps = 32.0 * (1 << self.n) / (ms * 1e-3) / 1e9
        return {"GBps": round(gbps, 1), "frac_of_8TBps": round(gbps / 8000.0, 4), "ms": round(ms, 4),
                "bytes": 32 * (1 << self.n), "kernel": "k_copy (read + write, non-temporal above 256 MiB)"}

    def stream_ceiling(self, reps: int = 5) -> dict:
        """What this device streams at the state's size in THIS run: the best of the copy kernel (non-temporal and plain),
        the runtime's device-to-device copy, and an in-place read-modify-write of every amplitude (H on a middle index
        bit: one 32-B round trip per amplitude, the access pattern of the gate kernels themselves).  All move 32 B per
        amplitude.  bench.py reports the fused pass against the best of them (`frac_of_achievable`): unlike the copy
        kernel alone (r04: 0.71 of peak while the in-place H reached 0.77 in the same run) the maximum IS a ceiling of
        what was seen to stream on this box."""
        other = DeviceChunk.empty(self.n, self.state.device)
        nbytes = 32.0 * (1 << self.n)
        H = gate_table.H()

        def timed(fn) -> float:
            fn()
            other.sync()
            ts = []
            for _ in range(reps):
                other.time_begin()
                fn()
                ts.append(other.time_end())
            return float(np.median(ts))
        other.copy_from(self.state)
        rows = {"copy_nontemporal": timed(lambda: other.copy_from(self.state, 1)),
                "copy_plain": timed(lambda: other.copy_from(self.state, 2)),
                "copy_hipMemcpyAsync": timed(lambda: other.copy_from(self.state, 3)),
                "inplace_rmw_H_bit12": timed(lambda: other.apply_1q(min(12, self.n - 1), H)),
                "inplace_rmw_H_bit5": timed(lambda: other.apply_1q(min(5, self.n - 1), H))}
        other.close()
        gbps = {name: round(nbytes / (ms * 1e-3) / 1e9, 1) for name, ms in rows.items()}
        best = max(gbps, key=gbps.get)
        return {"GBps": gbps[best], "best": best, "frac_of_8TBps": round(gbps[best] / 8000.0, 4), "candidates_GBps": gbps,
                "bytes": int(nbytes), "note": "each candidate moves 32 B per amplitude of a buffer of the state's size; median of %d" % reps}

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


def layout_swaps(cur, want, n: int) -> list:
    """Index-bit pairs whose SWAPs, applied in order, take a state from layout `cur` to layout `want` (logical qubit q on
    index bit layout[q]; None = identity): at most n - 1 of them."""
    cur = list(cur) if cur is not None else list(range(n))
    want = list(want) if want is not None else list(range(n))
    at = {p: q for q, p in enumerate(cur)}              # index bit -> the logical qubit on it
    swaps = []
    for q in range(n):
        a, b = cur[q], want[q]
        if a != b:
            other = at[b]                               # the qubit sitting where q has to go
            swaps.append((a, b))
            at[a], at[b] = other, q
            cur[other], cur[q] = a, b
    return swaps


def _count_passes(n: int, batches, layouts: np.ndarray, threads: int) -> np.ndarray:
    """Fused passes of the batches under each layout (rows of `layouts`: qubit -> index bit), planned on the host."""
    total = np.zeros(len(layouts), dtype=np.int64)
    for ops in batches:                                     # (a single op is not planned: one pass)
        total += planner.count_layouts(n, ops, layouts, threads) if len(ops) >= 2 else len(ops)
    return total


def choose_plan_layout(n: int, batches, n_candidates: int = 31, seed: int = 20260504, n_finalists: int = 4,
                       all_finalists: bool = False, beam: int = 0, engine_costs=None, priced_batches=None):
    """(l2p, tile masks per batch on the chosen index bits, info) for the op lists `batches` (logical qubits).  The three
    qubits on the line bits belong to every tile, so they decide how many passes a plan needs; which index bits the OTHER
    qubits live on does not (a relabelling of the bits >= 3 maps every valid pass sequence to a valid one).  So: for the
    identity and `n_candidates` random line-qubit triples the library's searching pass builder (qsim_plan_search, beam
    width `beam`, 0 = its default) plans the batches, in parallel on the host; the triples that need the fewest passes
    are kept and their other qubits placed by the tile-cost model (runner/tile_layout.py).  Host only.  all_finalists: the
    list of up to n_finalists minimum-pass layouts, best model cost first (the engine may time them on the device).
    engine_costs (the table of runner/engine_cost.py; None: pricing off): a pass is priced max(memory model of its tile,
    engine time of its records); `priced_variant` then chooses between `batches` and `priced_batches` (the same lists
    under rule (d) of the rewrite, optional) and places the ops that need no tile: info gains `planned` (the op lists to
    run, on their index bits), `placed` (their placements, per batch) and the modelled split (`model_split_ms`), and the
    finalists rank by that total instead of the memory model alone."""
    import os
    from concurrent.futures import ThreadPoolExecutor

    from quantum_simulations_amd import _lib
    from quantum_simulations_amd.runner import tile_layout
    rng = np.random.default_rng(seed)
    layouts = np.tile(np.arange(n, dtype=np.int32), (n_candidates + 1, 1))
    for row in layouts[1:]:
        for bit, q in enumerate(int(x) for x in rng.choice(n, size=3, replace=False)):
            j = int(np.flatnonzero(row == bit)[0])          # the qubit on `bit` trades places with q
            row[j], row[q] = row[q], bit
    try:
        threads = len(os.sched_getaffinity(0))
    except AttributeError:
        threads = os.cpu_count() or 1
    threads = max(1, min(16, threads))
    _lib.load()

    def relabelled(lay):
        return [[([int(lay[q]) for q in qs], U) for qs, U in ops] for ops in batches]

    def search(lay):                                        # (the library call releases the interpreter lock)
        none = np.zeros(0, dtype=np.uint64)
        return [planner.search_tiles(n, ops, beam) if len(ops) >= 2 else none for ops in relabelled(lay)]
    with ThreadPoolExecutor(threads) as pool:
        found = list(pool.map(search, layouts))
    short = sum(len(ops) for ops in batches if len(ops) < 2)                    # (a single op is not searched: one pass)
    counts = np.array([short + sum(len(ms) for ms in f) for f in found], dtype=np.int64)
    best = int(counts.min())
    finalists = [int(i) for i in np.flatnonzero(counts == best)][:max(1, n_finalists)]   # (the identity first when it ties)
    greedy_identity = int(_count_passes(n, batches, layouts[:1], 1)[0])
    out = []
    for f in finalists:
        first = [int(x) for x in layouts[f]]
        moved = relabelled(first)
        masks = found[f]
        tiles = [[b for b in range(tile_layout.LOW, n) if (int(m) >> b) & 1] for ms in masks for m in ms]
        second, cost0, cost1 = min((tile_layout.choose_layout(tiles, n, seed=s) for s in range(1, 9)), key=lambda r: r[2])
        final_masks = [np.array([sum(1 << second[b] for b in range(n) if (int(m) >> b) & 1) for m in ms], dtype=np.uint64) for ms in masks]
        # The pass count does not depend on the placement, but the records of a pass are written in the order of its tile
        # bits, and a pass at the edge of its record budget may hold one op fewer in another order: a placement that would
        # grow the plan at execution time is dropped for the one the search ran on.
        replanned = sum(planner.pass_count(n, [([second[b] for b in qs], U) for qs, U in ops], ms) if len(ops) >= 2 else len(ops)
                        for ops, ms in zip(moved, final_masks))
        if replanned != best:
            second, final_masks, cost1 = list(range(n)), [np.array(ms, dtype=np.uint64) for ms in masks], cost0
        l2p = [second[first[q]] for q in range(n)]
        info = {"passes_identity": greedy_identity, "passes_chosen": best, "candidates": n_candidates + 1,
                "candidates_by_passes": {int(c): int((counts == c).sum()) for c in np.unique(counts)},
                "passes_identity_searched": int(counts[0]), "beam": int(beam) if beam > 0 else "default",
                "model_ms": (round(cost0, 3), round(cost1, 3))}
        if engine_costs is not None:
            def on_bits(lists):
                return [[([l2p[q] for q in qs], U) for qs, U in ops] for ops in lists]
            # info["planned"]: the op lists the plan runs (on their index bits), info["placed"]: their placements
            info["planned"], info["placed"], info["model_split_ms"] = priced_variant(
                n, on_bits(batches), None if priced_batches is None else on_bits(priced_batches), final_masks, engine_costs)
            info["passes_chosen"] = info["model_split_ms"]["pass_count"]       # (a list under rule (d) may finish a pass early)
        out.append((l2p, final_masks, info))
    out.sort(key=lambda r: r[2]["model_split_ms"]["passes"] if "model_split_ms" in r[2] else r[2]["model_ms"][1])
    return out if all_finalists else out[0]


def pass_memory_us(n: int, masks) -> np.ndarray:
    """Microseconds the tile-cost model (runner/tile_layout.py) gives every pass of the tiles `masks` without its gates, on
    2^n amplitudes (the model's own state size scaled to n)."""
    from quantum_simulations_amd.runner import tile_layout
    model = tile_layout.model_for(n)
    scale = 2.0 ** (n - min(tile_layout._load_models(), key=lambda k: (abs(k - n), k)))
    return np.array([tile_layout.tile_cost(model, [b for b in range(tile_layout.LOW, n) if (int(m) >> b) & 1]) * scale * 1e3 for m in masks])


def priced_variant(n: int, batches, priced_batches, masks, engine_costs) -> tuple:
    """(batches kept, placement per batch, model split): the cheaper of the plans the SAME tiles `masks` (one mask array
    per batch; the batches already on their index bits) give -- `batches` run first come, which is the plan with the
    pricing off, against `priced_batches` (the same lists under rule (d) of the rewrite; may be None) and `batches`
    themselves with their ops that need no tile placed by `planner.balance`.  A candidate is taken when it needs no more
    passes than the unpriced plan and the model prices it lower, so a priced plan never has a pass more and is never
    modelled dearer.  The split (milliseconds summed over the passes): `memory` (the tile model), `engine` (the records by
    the table), `passes` (sum of max(memory, engine)), `passes_unpriced` (the same of the unpriced plan); `pass_count`,
    `moved_ops` (placed later than first come) and `rule_d_ops` (ops rule (d) removed; 0: `batches` kept)."""
    mems = [pass_memory_us(n, ms) for ms in masks]

    def price(lists, place):
        tot = {"memory": 0.0, "engine": 0.0, "passes": 0.0, "pass_count": 0, "moved_ops": 0}
        placed = []
        for ops, ms, mem in zip(lists, masks, mems):
            if len(ops) < 2 or not len(ms):                 # (a single op is not planned: one pass, not priced)
                placed.append(None)
                tot["pass_count"] += len(ops)
                continue
            earliest, before, after = planner.balance(n, ops, ms, mem, engine_costs, place)
            placed.append(earliest if earliest is not None and earliest.any() else None)
            tot["memory"] += mem.sum() / 1e3
            tot["engine"] += after.sum() / 1e3
            tot["passes"] += np.maximum(mem, after).sum() / 1e3
            tot["pass_count"] += planner.pass_count(n, ops, ms, placed[-1])
            tot["moved_ops"] += 0 if placed[-1] is None else int((placed[-1] > 0).sum())
        return tot, placed

    def shown(tot, **more):
        return dict({k: (round(float(v), 6) if isinstance(v, float) else int(v)) for k, v in tot.items()}, **more)
    plain, none_placed = price(batches, False)
    for lists in ([priced_batches] if priced_batches is not None else []) + [batches]:
        tot, placed = price(lists, True)
        if tot["pass_count"] <= plain["pass_count"] and tot["passes"] < plain["passes"]:
            removed = sum(len(a) - len(b) for a, b in zip(batches, lists))
            return lists, placed, shown(tot, passes_unpriced=round(float(plain["passes"]), 6), rule_d_ops=removed)
    return batches, none_placed, shown(plain, passes_unpriced=round(float(plain["passes"]), 6), rule_d_ops=0)


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
