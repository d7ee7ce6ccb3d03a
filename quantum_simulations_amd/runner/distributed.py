"""Multi-GPU engine: the 2^n amplitude vector partitioned by its high qubit bits, one process
per GPU (`torch.distributed`; backend "nccl" = RCCL over xGMI on the GPU node, "gloo" in the
CPU tests).

Rank g holds amplitudes [g*2^k, (g+1)*2^k): the reference's chunk g (block_store.py:14-15),
so a gate on qubit q >= k pairs rank g with g XOR 2^(q-k) exactly like partner chunks
(cpu_nonlocal.py:7-15, single_node.py:271-321).  This module replaces the Spark/HiSVSIM chunk
partitioner and the driver-side sequential partner-group loop (spark_runner.py:148-194):

  local gates ....................... HIP kernels on the shard, no communication
  diagonal gate, global qubit(s) .... phase chosen by the rank's own bits, NO exchange
                                       (the reference runs these as butterflies, staging.py:67-72)
  controlled gate, global control ... ranks whose control bit is 1 apply the 1q gate (locally,
                                       or with one partner when the target is global too)
  (local ops produced by the two rows above are queued and fused into the next local pass)
  other gates on a global qubit ..... swap-and-stay: the global qubit trades places with a local one
                                       that is not needed soon (HALF a shard over one xGMI link for one
                                       global qubit, 3/4 over three links for two), the gate then runs
                                       locally in the next fused pass and the layout change is tracked
                                       (the arithmetic of cpu_nonlocal.py:22-67 / single_node.py:271-321
                                       without shipping whole shards there and results back)
  staging SWAP lists ([p_out<k, p_in>=k], SWAP; staging.py:136-152) of one step are MERGED
  into ONE all-to-all re-layout: each rank packs 2^m - 1 slabs, exchanges them with 2^m - 1
  peers concurrently (all links busy) and unpacks in place.

The communication schedule lives here, in Python, and is backend-agnostic; all arithmetic on
amplitudes is done by a shard backend (runner/shard_backends.py; HIP: `HipShardBackend`; the CPU
test double lives in tests/ and is never selected by the product).  This file is the schedule alone:
`execute` -> `run_step` -> `relayout` / `apply_nonlocal` -> `_run_local` -> `_post` / `_finish`.  Plans and
the start layout: runner/distributed_plan.py; readout, self-checks and the timed BASELINE configurations:
runner/distributed_checks.py (both are bases of `DistributedEngine`).
"""
from __future__ import annotations

import numpy as np

from quantum_simulations_amd.kernel import gates as gate_table
from quantum_simulations_amd.runner.distributed_checks import ChecksMixin
from quantum_simulations_amd.runner.distributed_plan import Plan, PlanningMixin
# (re-exported: tests and callers outside the package take the backends and `Plan` from here)
from quantum_simulations_amd.runner.shard_backends import DryBackend, HipShardBackend, PlanningBackend, split_pieces  # noqa: F401

_SWAP = gate_table.SWAP()
_I2 = np.eye(2, dtype=np.complex128)


# ------------------------------------------------------------------ gate structure tests
def _is_diagonal(U: np.ndarray) -> bool:
    return not np.any(U - np.diag(np.diag(U)))


def _controlled_on_first(U: np.ndarray):
    """4x4 = |0><0| x I + |1><1| x V (control = qubits[0]) -> V, else None."""
    if np.array_equal(U[:2, :2], _I2) and not np.any(U[:2, 2:]) and not np.any(U[2:, :2]):
        return U[2:, 2:].copy()
    return None


def _controlled_on_second(U: np.ndarray):
    """Control = qubits[1] (identity on pair indices {0,2}, V on {1,3}) -> V, else None."""
    P = U[np.ix_([0, 2, 1, 3], [0, 2, 1, 3])]
    return _controlled_on_first(P)


class DistributedEngine(PlanningMixin, ChecksMixin):
    def __init__(self, n_qubits: int, world: int, rank: int, local_rank: int = 0, mode: str = "fused", backend=None,
                 staging: bool = True, staging_method: str = "tiles", init_process_group: bool = True,
                 relayout_pieces: int = 4, min_piece_qubits: int = 20, fuse_relayout: bool = True,
                 rehearsal: bool = False, exchange: str = "torch", layout: str = "auto", pipeline_relayout: bool = True):
        import torch
        import torch.distributed as dist
        self.torch, self.dist = torch, dist
        if world & (world - 1) or world < 1:
            raise ValueError("world size must be a power of two")      # (1: no global qubit, nothing is ever exchanged: plumbing tests)
        self.n, self.world, self.rank = n_qubits, world, rank
        self.p = world.bit_length() - 1
        self.k = n_qubits - self.p
        if self.k < 2:
            # a dense gate on global qubits is brought local by trading places with local qubits (swap-and-stay): a
            # 2-qubit gate needs two local places; shards of fewer than 4 amplitudes are not supported
            raise ValueError(f"{n_qubits} qubits on {world} ranks leave {max(self.k, 0)} local qubit(s): at least 2 are needed "
                             "(use fewer ranks)")
        self.mode, self.staging, self.staging_method = mode, staging, staging_method
        self.tiles_min_ops = 0       # staging method "tiles": 0 = search the thin-pass threshold (plan_partition_best)
        self.plan_threads = 8
        self._plan_effort_high = False
        self.place_slots = True      # staging method "tiles", fresh state: local slots placed by the tile-cost model
        self.place_slots_min_k = 26  # (the model was fitted at 28 / 30 qubits; smaller shards are cache resident: tests lower it)
        self.use_tile_hints = True
        # rehearsal (explicit argument; bench.py --rehearsal): several ranks share the visible GPU(s), each with its shard
        # in HBM and the real HIP kernels, and exchange through host-staged gloo -- RCCL refuses two ranks on one
        # device.  `self.exchange` names what carries the transfers and is printed in every bench line.
        rehearsal = bool(rehearsal) and backend is None
        if backend is None:
            if rehearsal:
                local_rank = local_rank % max(1, torch.cuda.device_count())
            torch.cuda.set_device(local_rank)     # before RCCL initialises: one rank <-> one GPU
        if init_process_group and not dist.is_initialized():
            if backend is None and not rehearsal:
                dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device(f"cuda:{local_rank}"))
            else:
                dist.init_process_group("gloo", rank=rank, world_size=world)
        if exchange not in ("torch", "cabi"):
            raise ValueError("exchange must be 'torch' (torch.distributed P2P) or 'cabi' (qsim_comm_exchange)")
        self.exchange_api = exchange
        self.exchange = "gloo-rehearsal" if rehearsal else ("rccl" if backend is None else f"gloo ({type(backend).__name__})")
        self.backend = backend if backend is not None else HipShardBackend(self.k, local_rank)
        if exchange == "cabi":
            # the transfers are posted by the library's own RCCL communicator (qsim_comm_exchange_bg on its transfer
            # stream) instead of torch.distributed P2P: the same schedule, the path a C-only host uses
            if rehearsal or not hasattr(self.backend, "comm_init"):
                raise ValueError("exchange='cabi' needs one rank per GPU and the HIP backend (RCCL inside libqsim_hip.so)")
            self.backend.comm_init(dist, rank, world)
        self.dry = bool(getattr(self.backend, "dry", False))
        self.trace: list | None = [] if self.dry else None     # dry runs: (kind, peer, sent, received) per posted transfer
        self.trace_posts = 0                                   # dry runs: groups posted (>= 2 per fused re-layout: pieces)
        self.l2p_planned = list(range(n_qubits))   # logical qubit -> physical index bit as the PLANS see it
        self._dyn = list(range(n_qubits))          # planned physical bit -> actual physical bit (swap-and-stay moves)
        self._flat: list = []                      # qubit lists of the running execution, in order (victim choice)
        self._flat_pos = 0
        self.xgmi_bytes_sent, self.exchanges, self._comm_events = 0, 0, []
        if relayout_pieces not in (1, 2, 4, 8):
            raise ValueError("relayout_pieces must be 1, 2, 4 or 8")
        self.relayout_pieces, self.min_piece_qubits = relayout_pieces, min_piece_qubits
        # Initial qubit layout: the first plan after `init_zero_state` may start from any assignment of qubits to index bits
        # and searches for a cheap one (runner/distributed_plan.py: staging method "tiles" prices a few with the partition
        # planner, deterministically on every rank; the other methods execute LAYOUT_CANDIDATES on a planning twin).
        # "auto": shards of >= 20 local qubits (staged or swap-and-stay schedules alike); "search": always (tests); "identity": never.
        if layout not in ("auto", "search", "identity"):
            raise ValueError("layout must be 'auto', 'search' or 'identity'")
        self.layout = layout
        self._fresh = False                        # the state is |0..0> and no plan has chosen a layout for it yet
        self._shadow = None                        # (the planning twin that prices candidate layouts, made on first use)
        self.relayout_log: list = []               # slab-bit counts of the re-layouts made since the last reset (shadow engines)
        self.layout_info = None
        self._passes = self.last_passes = 0
        self.home_moves = 0                        # times "state" and "buf1" traded names (one-pass op list between two re-layouts)
        self._pending: list = []
        self._pending_tiles: list = []             # tile masks the planner named for the passes of the queued ops
        # Re-layout fused with the neighbouring local passes (`relayout`): no separate pack / unpack pass of the shard.
        # `_state_in` = (buffer, local bits) while the shard lives in a receive buffer in slab layout (None: in "state", index
        # order); `_inflight` = (posted groups, timer) while the pieces of that re-layout may still be on the links: the next
        # reader of the shard consumes them piece by piece (`_run_local`).
        self.fuse_relayout = fuse_relayout
        self._state_in = self._inflight = None
        # pipeline_relayout = False (bench.py --no-relayout-pipeline): the plain form of a fused re-layout -- whole slabs
        # stored by one launch, ONE group posted, and the host path WAITS for it before anything reads the shard (no pieces,
        # nothing left `_inflight`).  The in-flight piece pipeline has only ever run on one GPU and under gloo rehearsal: a
        # first multi-GPU run that fails can be repeated with this switch to tell a wrong schedule from an ordering problem
        # between the transfer stream and the partial launches.
        self.pipeline_relayout = bool(pipeline_relayout)
        # Memory per rank: the shard + the send buffer + the receive buffer = 3 shard-sized allocations (48 GiB at 30 local
        # qubits, 192 GiB at 32), fused re-layouts or not (`relayout`: the buffers trade names).  Claimed here, not in the
        # middle of a circuit.
        if not self.dry and hasattr(self.backend, "tensor"):
            try:
                for name in ("buf0", "buf1"):
                    self.backend.tensor(name)
            except RuntimeError as e:        # torch's out-of-memory error is a RuntimeError
                raise MemoryError(f"rank {rank}: no room for the exchange buffers (3 x {16 << self.k} bytes per rank are "
                                  f"needed): {e}") from e

    # ---- helpers -----------------------------------------------------------------------
    @property
    def l2p(self) -> list[int]:
        """logical qubit -> ACTUAL physical index bit (planned layout composed with the dynamic moves)"""
        return [self._dyn[p] for p in self.l2p_planned]

    def _rank_bit(self, phys_qubit: int) -> int:
        return (self.rank >> (phys_qubit - self.k)) & 1

    def _reduce(self, values, op=None) -> np.ndarray:
        """Collective: `values` (float64s) summed -- or combined by `op` -- over the ranks.  (Under "nccl" the numbers cross
        on the shard's device, here and in `_gather`.)"""
        t = self.torch.tensor(values, dtype=self.torch.float64)
        t = t.to(self.backend.tensor("state").device) if self.dist.get_backend() == "nccl" else t
        self.dist.all_reduce(t, op=self.dist.ReduceOp.SUM if op is None else op)
        return t.cpu().numpy()

    def _gather(self, values) -> list:
        """Collective: every rank's `values` (float64s, the same count on all), in rank order."""
        t = self.torch.as_tensor(values, dtype=self.torch.float64)
        t = t.to(self.backend.tensor("state").device) if self.dist.get_backend() == "nccl" else t
        parts = [self.torch.empty_like(t) for _ in range(self.world)]
        self.dist.all_gather(parts, t)
        return [p.cpu().numpy() for p in parts]

    def _post(self, send: str, recv: str, entries):
        """Post entries [(peer, start, count)] together -- `count` float64 elements at offset `start` of buffer `send` go
        to `peer`, as many arrive from it at the same place of `recv` -- without waiting (RCCL: the group is ordered after
        everything already queued on the shard's stream and runs beside what is queued later).  One group = every peer
        at once: all links busy."""
        dist, torch = self.dist, self.torch
        if self.dry:
            self.trace_posts += 1
            for peer, start, count in entries:
                self.backend.tensor(send)[start:start + count]          # (slice bounds are checked)
                self.backend.tensor(recv)[start:start + count]
                self.trace.append((self._trace_kind, int(peer), count * 8, count * 8))
                self.xgmi_bytes_sent += count * 8
            return ([], [])
        if not entries:
            return ([], [])
        self.xgmi_bytes_sent += sum(c for _, _, c in entries) * 8
        if self.exchange_api == "cabi":
            ticket = self.backend.exchange_bg(send, recv, [(peer, start // 2, count // 2) for peer, start, count in entries])
            return ("cabi", ticket)
        st, rt = self.backend.tensor(send), self.backend.tensor(recv)
        staged, ops = [], []
        host = dist.get_backend() == "gloo"
        for peer, start, count in entries:
            s_t, r_t = st[start:start + count], rt[start:start + count]
            if host and s_t.is_cuda:   # rehearsal of several ranks on one GPU: stage through host
                s_h, r_h = s_t.cpu(), torch.empty(r_t.shape, dtype=r_t.dtype)
                staged.append((r_t, r_h))
                s_t, r_t = s_h, r_h
            ops.append(dist.P2POp(dist.isend, s_t, peer))
            ops.append(dist.P2POp(dist.irecv, r_t, peer))
        return (dist.batch_isend_irecv(ops), staged)

    def _finish(self, posted) -> None:
        """Received data may be used by what is queued after this (RCCL: the shard's stream waits, not the host)."""
        works, staged = posted
        if works == "cabi":
            self.backend.exchange_wait(staged)
            return
        for work in works:
            work.wait()
        for dev_t, host_t in staged:
            dev_t.copy_(host_t)

    _trace_kind = "relayout"

    def _comm_timer(self, tensor):
        """Device-side time of an exchange (stream events, summed in comm_stats)."""
        if not (tensor.is_cuda and self.dist.get_backend() == "nccl"):
            return None
        ev0, ev1 = self.torch.cuda.Event(enable_timing=True), self.torch.cuda.Event(enable_timing=True)
        ev0.record()
        return ev0, ev1

    def _comm_done(self, timer) -> None:
        if timer is not None:
            timer[1].record()
            self._comm_events.append(timer)
        self.exchanges += 1

    # ---- deferred local work -------------------------------------------------------------------
    # Global-qubit gates that need no exchange end up as LOCAL ops on this rank (a rank-bit phase,
    # a diagonal on the local partner qubit, the conditional 1q gate of a global control).  Run one
    # by one each is a full HBM pass of the shard; queued, they ride in the next fused local pass
    # (program order is kept: they sit between two local batches), or are flushed before anything
    # that reads the shard (an exchange, a re-layout, a reduction, a download).
    def _queue_local(self, op) -> None:
        self._fresh = False
        self._pending.append(op)

    def _run_local(self, ops, dst=None, parts: int = 0) -> None:
        """`ops` (may be empty) on the shard wherever it lives -- in "state", in a receive buffer in slab layout
        (`_state_in`), or still arriving there piece by piece (`_inflight`): then the backend plans now and every piece
        is handed over as soon as its transfer is done (torch: the shard's stream waits for that group, not the host), so
        the first pass runs on the tiles whose pieces are there while the later pieces are on the links.  `dst` / `parts`:
        the slab-storing end of the next re-layout."""
        src = self._state_in
        kw = {}
        if self._pending_tiles:          # (the partition planner's tiles for this op list: staging method "tiles")
            kw["tiles"], self._pending_tiles = np.array(self._pending_tiles, dtype=np.uint64), []
        if src is None:
            if dst is None:
                if ops:
                    self._passes += self.backend.apply_ops(ops, **kw) or 0
            else:
                self._passes += self.backend.apply_ops(ops, dst=dst, parts=parts, **kw) or 0
            return
        self._state_in = None
        if self._inflight is None:
            self._passes += self.backend.apply_ops(ops, src=src, dst=dst, parts=parts, **kw) or 0
            return
        self._passes += self.backend.apply_ops(ops, src=src, dst=dst, parts=parts, src_parts=self._split_parts(), **kw) or 0
        self._drain_inflight(self.backend.load_part)

    def _flush_local(self) -> None:
        """Run the queued local ops (reading the shard from the receive buffer it may still live in, or be arriving in);
        with nothing queued a shard that is not at home is brought there (unpack pieces)."""
        if self._pending or self._state_in is not None:
            ops, self._pending = self._pending, []
            self._run_local(ops)

    def _drain_inflight(self, on_piece=None) -> None:
        """Finish the transfers that still write into the exchange buffers, in the order they were posted (`on_piece(j)`
        right after group j: `_run_local` tells the backend that piece j is there); without `on_piece`: the state is about
        to be overwritten, or a plain re-layout waits for its one group."""
        if self._inflight is not None:
            (posted, timer), self._inflight = self._inflight, None
            for j, pst in enumerate(posted):
                self._finish(pst)
                if on_piece is not None:
                    on_piece(j)
            self._comm_done(timer)

    # ---- state ---------------------------------------------------------------------------
    def init_zero_state(self) -> None:
        self._drain_inflight()
        self._pending, self._pending_tiles, self._state_in = [], [], None
        self.backend.init_zero(self.rank == 0)
        self.l2p_planned, self._dyn = list(range(self.n)), list(range(self.n))
        self._fresh = True
        self.layout_info = None

    # ---- execution ---------------------------------------------------------------------------
    def execute(self, plan: Plan) -> None:
        i = plan.cursor
        if i >= len(plan.executions):
            raise RuntimeError("plan exhausted: call engine.plan(circuit, repeats=K) with enough repeats")
        if plan.start_mappings[i] != self.l2p_planned:
            raise RuntimeError("this execution of the plan was planned for another qubit layout than the engine's "
                               "current one (the state was re-initialised or another plan ran in between): re-plan")
        self._passes = 0
        self._flat = [qs for step in plan.executions[i] for qs, _ in list(step["local_ops"]) + list(step["nonlocal_ops"])]
        self._flat_pos = 0
        for step in plan.executions[i]:
            self.run_step(step)
        self._flush_local()
        self.last_passes = self._passes
        self.l2p_planned = list(plan.mappings[i])
        plan.cursor = i + 1

    def _actual(self, qs) -> list[int]:
        return [self._dyn[q] for q in qs]

    def run_step(self, step: dict) -> None:
        """Ops carry PLANNED physical bits; swap-and-stay moves may have put a planned-local qubit on a
        rank bit (and back), so every op is classified by where its qubits actually are."""
        k = self.k
        self._fresh = False              # (the state is no longer |0..0>: no later plan may pick another layout for it)
        if step.get("tile_masks") and self.use_tile_hints:
            self._pending_tiles += [int(m) for m in step["tile_masks"]]
        batch = []
        for qs, U in step["local_ops"]:
            aq = self._actual(qs)
            if all(q < k for q in aq):
                batch.append((aq, U))
            else:                                   # a victim of an earlier move: the ops before it first
                self._pending += batch
                batch = []
                self.apply_nonlocal(aq, U)
            self._flat_pos += 1
        self._pending += batch           # runs with the next flush: before an exchange (whose pack it then absorbs),
        ops = step["nonlocal_ops"]       # a reduction, a download, or at the end of the execution
        i = 0
        while i < len(ops):
            j = i
            group = []
            used: set[int] = set()
            while (j < len(ops) and len(group) < 3 and self._is_planned_swap(ops[j])
                   and self._is_cross(self._actual(ops[j][0])) and used.isdisjoint(self._actual(ops[j][0]))):
                group.append(self._actual(ops[j][0]))   # (at most 3 pairs: qsim_pack_all's slab patterns)
                used.update(group[-1])
                j += 1
            if group:
                self.relayout(group)
                self._flat_pos += j - i
                i = j
                continue
            qs, U = ops[i]
            if self._is_planned_swap(ops[i]):
                # a planned SWAP whose qubits are on the same side now: nothing has to move -- the two
                # planned positions trade their actual bits (later gates find the qubits where they are)
                a, b = qs
                self._dyn[a], self._dyn[b] = self._dyn[b], self._dyn[a]
            else:
                aq = self._actual(qs)
                if all(q < k for q in aq):
                    self._queue_local((aq, U))
                else:
                    self.apply_nonlocal(aq, U)
            self._flat_pos += 1
            i += 1

    def _is_cross(self, aq) -> bool:
        return (aq[0] < self.k) != (aq[1] < self.k)

    @staticmethod
    def _is_planned_swap(op) -> bool:
        qs, U = op
        return len(qs) == 2 and U.shape == (4, 4) and np.array_equal(U, _SWAP)

    # -- all-to-all re-layout: swap m local bits with m global bits ------------------------------
    def relayout(self, pairs) -> None:
        """pairs: [[p_a, p_b], ...] each with exactly one local and one global physical bit.

        Fused (the default, slab bits above the line bits): the queued local ops' last pass stores the slabs, one
        grouped exchange of whole slabs, the next local pass loads them -- no pass of the shard outside the links.
        Unfused: pack / exchange / unpack, pipelined in `pieces` sub-ranges of every slab (while piece s is on the
        links, piece s+1 is being packed and piece s-1 unpacked)."""
        self._fresh = False
        loc, glo, m = [min(p) for p in pairs], [max(p) for p in pairs], len(pairs)
        self.relayout_log.append(m)
        mine, peers, slab = self._slab_peers(glo)
        send = self.backend.tensor("buf0")
        pieces = self._relayout_pieces(self.k - m)
        part = slab // pieces
        if self.fuse_relayout and min(loc) >= 3 and self.k - m >= 3:
            # (A slab bit inside a 128-byte line would break whole-line accesses: the unfused path below handles it.)
            # What overlaps what: the slab-storing pass is cut into up to `relayout_pieces` PIECES (the j-th equal sub-range
            # of every slab: qsim_ops_io::dst_parts) and the exchange of piece j -- one group with all 2^m - 1 peers, every
            # link busy -- is posted as soon as piece j is stored, so it travels while the pieces behind it are computed;
            # only the first piece's compute and the last piece's transfer are exposed on the send side.  The cut depends
            # only on (k, m, pieces): all ranks post the same messages in the same order whatever their own pass plans look
            # like (a rank whose last pass holds a piece bit as a tile bit has all its pieces ready at once: it overlaps less,
            # it does not post differently).  The first pass AFTER the exchange takes the pieces over as they arrive
            # (`_inflight`, qsim_ops_io::src_parts): it runs on the tiles whose pieces are there -- when the piece bits are no
            # tile bits of it -- while the later pieces are on the links.
            # Buffers: the slabs go into "buf0", the slab that stays straight into the receive buffer "buf1" -- also when
            # the shard currently LIVES in "buf1" (two re-layouts with little between them): with two or more kernels "buf1"
            # has been consumed by the first before the last stores into it; when ONE pass reads "buf1" and stores the
            # slabs, the library leaves the own slab in "state" instead (nobody needs its contents then), the exchange
            # delivers into "state", and "state" and "buf1" trade names afterwards: the shard is in "buf1" again and the
            # consumed buffer is the new home.  Three shard-sized buffers per rank in every case.
            from_recv = self._state_in is not None and self._state_in[0] == "buf1"
            ops, self._pending = self._pending, []
            piped = self.pipeline_relayout
            if not piped:                 # plain form: nothing of an earlier re-layout stays in flight
                self._drain_inflight()
            self._run_local(ops, dst=("buf0", loc, "buf1", mine), parts=self._split_parts() if piped else 0)
            rname = "state" if (from_recv and self.backend.own_slab_in_state()) else "buf1"
            timer = self._comm_timer(send)
            if piped:                     # one group per piece, posted as soon as the piece is stored
                posted = []
                for j, (off, cnt) in enumerate(self.backend.pending_parts()):
                    self.backend.store_part(j)
                    posted.append(self._post("buf0", rname, [(peer, d * slab + 2 * off, 2 * cnt) for d, peer in peers]))
            else:                         # plain form: the slabs were stored by that call, one group carries them whole
                posted = [self._post("buf0", rname, [(peer, d * slab, slab) for d, peer in peers])]
            # nobody waits here: the next reader of the shard takes the pieces over as they arrive (_run_local)
            self._inflight = (posted, timer)
            if not piped:                 # plain form: the host path waits now, before anything reads the shard
                self._drain_inflight()
            if rname == "state":
                self.backend.swap_names("state", "buf1")       # (posted transfers hold the buffers themselves, not the names)
                self.home_moves += 1
            self._state_in = ("buf1", list(loc))
            return
        self._flush_local()
        self._passes += 2
        timer = self._comm_timer(send)
        posted = []
        self.backend.pack_all(loc, "buf0", mine, 0, pieces)        # slab d at offset d * 2^(k-m)
        for s in range(pieces):
            posted.append(self._post("buf0", "buf1", [(peer, d * slab + s * part, part) for d, peer in peers]))
            if s + 1 < pieces:
                self.backend.pack_all(loc, "buf0", mine, s + 1, pieces)
        for s in range(pieces):
            self._finish(posted[s])
            self.backend.unpack_all(loc, "buf1", mine, s, pieces)
        self._comm_done(timer)

    def _slab_peers(self, glo) -> tuple:
        """(mine, peers, slab) of an all-to-all over the rank bits `glo`: the pattern this rank's own bits make (the slab
        that stays), [(pattern d, rank that gets slab d)] for every other pattern in rising order, float64 elements per slab."""
        k, mine = self.k, sum(self._rank_bit(g) << i for i, g in enumerate(glo))
        peers = []
        for d in range(1 << len(glo)):
            if d != mine:
                peer = self.rank
                for i, g in enumerate(glo):
                    peer = (peer & ~(1 << (g - k))) | (((d >> i) & 1) << (g - k))
                peers.append((d, peer))
        return mine, peers, 2 << (k - len(glo))

    def _split_parts(self) -> int:
        """qsim_ops_io::dst_parts / src_parts of a fused re-layout: the configured pieces (the library keeps a piece >=
        2^20 amplitudes); negative (no floor) when the engine was built with a lower floor (tests on small shards)."""
        want = self.relayout_pieces
        return want if self.min_piece_qubits >= 20 else -want

    def _relayout_pieces(self, slab_qubits: int) -> int:
        """Pieces per slab: the configured count, capped so that a piece keeps >= 2^20 amplitudes
        (16 MiB per peer and piece -- large enough for full link rate)."""
        want = self.relayout_pieces
        while want > 1 and slab_qubits - (want.bit_length() - 1) < self.min_piece_qubits:
            want //= 2
        return max(1, want)

    # -- one gate with at least one global qubit ---------------------------------------------------
    def apply_nonlocal(self, qs, U) -> None:
        """qs: ACTUAL physical bits, at least one >= k."""
        k = self.k
        self._fresh = False
        if len(qs) == 1:
            q = qs[0]
            b = self._rank_bit(q)
            if _is_diagonal(U):                       # rank-bit phase, no exchange
                if U[b, b] != 1:
                    self._scale(U[b, b])
                return
            (v,) = self._bring_local([q], exclude=())
            self._queue_local(([v], U))
            return
        qa, qb = qs
        a_glob, b_glob = qa >= k, qb >= k
        if _is_diagonal(U):                           # CZ / CR / any diagonal: no exchange
            d = np.diag(U).reshape(2, 2)              # d[bit a][bit b]
            if a_glob and b_glob:
                f = d[self._rank_bit(qa), self._rank_bit(qb)]
                if f != 1:
                    self._scale(f)
            elif a_glob:
                row = d[self._rank_bit(qa)]
                if not (row[0] == 1 and row[1] == 1):
                    self._queue_local(([qb], np.diag(row)))
            else:
                col = d[:, self._rank_bit(qb)]
                if not (col[0] == 1 and col[1] == 1):
                    self._queue_local(([qa], np.diag(col)))
            return
        V = _controlled_on_first(U)
        ctrl, tgt = qa, qb
        if V is None:
            V = _controlled_on_second(U)
            ctrl, tgt = qb, qa
        if V is not None and ctrl >= k:               # global control: conditional 1q gate
            if tgt < k:
                if self._rank_bit(ctrl):
                    self._queue_local(([tgt], V))
            elif _is_diagonal(V):
                if self._rank_bit(ctrl):
                    self.apply_nonlocal([tgt], V)
            else:
                # the target has to come local on EVERY rank (the move is collective); the gate keeps its
                # global control and is applied by the ranks whose control bit is 1
                (v,) = self._bring_local([tgt], exclude=())
                if self._rank_bit(ctrl):
                    self._queue_local(([v], V))
            return
        # dense: every global qubit of the gate trades places with a local one, then the gate is local
        moved = self._bring_local([q for q in (qa, qb) if q >= k], exclude=[q for q in (qa, qb) if q < k])
        it = iter(moved)
        self._queue_local(([next(it) if qa >= k else qa, next(it) if qb >= k else qb], U))

    def _bring_local(self, glob, exclude) -> list[int]:
        """Swap-and-stay: the global actual bits `glob` trade places with local bits that are not needed
        for the longest time; returns the local bits that now hold them.  Half a shard crosses one link for
        one bit (3/4 over three links for two) and nothing is sent back: `_dyn` records the move."""
        victims = self._pick_victims(len(glob), set(exclude))
        self._trace_kind = "swap-and-stay"
        self.relayout([[v, g] for v, g in zip(victims, glob)])
        self._trace_kind = "relayout"
        # an UNPLANNED move: the contents of the swapped actual positions have traded places, the plans
        # do not know (a planned re-layout moves planned and actual positions alike: no update there)
        swap = {}
        for v, g in zip(victims, glob):
            swap[v], swap[g] = g, v
        self._dyn = [swap.get(a, a) for a in self._dyn]
        return victims

    def _pick_victims(self, count: int, exclude: set) -> list[int]:
        """Local actual bits whose next use in the running execution is farthest away (never: best).  Bits inside a
        128-byte line (0..2) come last: a slab over one of them moves 16 B per line (several times slower to pack,
        tools/relayout_probe.py) and cannot ride in a fused pass."""
        if self.k - len(exclude) < count:
            raise ValueError("not enough local qubits to bring a global gate local")
        planned_of = {a: p for p, a in enumerate(self._dyn)}
        next_use = {}
        want = {planned_of[b] for b in range(self.k) if b not in exclude}
        flat = self._flat
        for pos in range(self._flat_pos + 1, len(flat)):
            for q in flat[pos]:
                if q in want and q not in next_use:
                    next_use[q] = pos
            if len(next_use) == len(want):
                break
        cands = [b for b in range(self.k) if b not in exclude]
        cands.sort(key=lambda b: (b < 3, -next_use.get(planned_of[b], 1 << 60), -b))
        return cands[:count]

    def _scale(self, f) -> None:
        self._queue_local(([0], f * _I2))

    # ---- synchronisation ------------------------------------------------------------
    def barrier(self) -> None:
        self._flush_local()
        self.backend.sync()
        self.dist.barrier()

    def max_over_ranks(self, value: float) -> float:
        return float(self._reduce([value], self.dist.ReduceOp.MAX)[0])

    def close(self) -> None:
        self.backend.close()
        if self.dist.is_initialized():
            self.dist.barrier()
            self.dist.destroy_process_group()
