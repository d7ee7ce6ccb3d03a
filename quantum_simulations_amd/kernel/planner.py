"""The host planner of libqsim_hip.so in Python: what the pass builder would do with an op list, without a device
(csrc/abi_plan.h: qsim_plan_ops, qsim_lower_pass_images, qsim_plan_ops_tiled, qsim_plan_ops_placed, qsim_plan_balance, qsim_plan_search, qsim_plan_search_triples, qsim_plan_search_cycle, qsim_plan_count_layouts, qsim_plan_peek_pass,
qsim_rewrite_ops_priced; csrc/tile_launch.h: qsim_tiles_per_workgroup; csrc/abi_rotation.h: qsim_plan_pauli_rotations).

A thin binding.  `ops` is [(qubits, U), ...] or the tuple `pack_ops` returns (`device.as_packed`).  Return codes become
the exceptions of `_lib.check` and nothing else is read into them: what a caller makes of a list too short to plan is
the caller's business.  No module-level state: the layout search and the partition planner call in from thread pools
(the calls go through the `ctypes.CDLL` of `_lib.load()`, which releases the interpreter lock while the library runs).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from quantum_simulations_amd import _lib
from quantum_simulations_amd._lib import ptr
from quantum_simulations_amd.kernel.device import as_packed

IMAGE_BYTES = 4096                 # QSIM_PASS_IMAGE_BYTES (include/qsim_hip.h)
STREAM_OFF = 192                   # byte offset of the first record (csrc/tile_kernel.h kTileStreamOff)
# One pass image = the kernel-argument block `TileArgs` of k_tile (csrc/tile_kernel.h), field by field
PASS_IMAGE = np.dtype([("amp", "<u8"), ("nrec", "<i4"), ("T", "<i4"), ("h", "u1", (11,)), ("order", "u1"), ("ntiles", "<u4"),
                       ("lay_in", "u1", (12,)), ("lay_out", "u1", (12,)), ("amp_out", "<u8"),
                       # re-layout fused into a pass (planned images carry none: all zero)
                       ("amp_out_own", "<u8"), ("own_mask", "<u8"), ("own_value", "<u8"),
                       ("slab_in", "u1", (40,)), ("slab_out", "u1", (40,)), ("nbits", "u1"), ("perm", "u1"), ("reserved", "u1", (22,)),
                       ("stream", "u1", (IMAGE_BYTES - STREAM_OFF,))])
assert PASS_IMAGE.itemsize == IMAGE_BYTES
_FIRST_BUFFER = 64                 # images the first call of `plan_ops` has room for


def tile_bits(image) -> list:
    """The high tile bits of a pass (ascending; the line bits 0..2 belong to every tile and are not listed)."""
    return [int(b) for b in image["h"][:int(image["T"]) - 3]]


def tile_masks(images) -> np.ndarray:
    """`tile_bits` of every pass as one uint64 mask each: what `search_tiles` returns and the `tiles` arguments take."""
    return np.array([sum(1 << b for b in tile_bits(img)) for img in images], dtype=np.uint64)


def _plan(n: int, ops, tiles, images, earliest=None) -> tuple:
    """(return code, pass count) of one qsim_plan_ops / qsim_plan_ops_tiled / qsim_plan_ops_placed call; `images`: None to
    count only."""
    nq, qubits, mats = as_packed(ops)
    lib, count = _lib.load(), C.c_int32()
    head = (n, len(nq), ptr(nq), ptr(qubits), ptr(mats))
    tail = (ptr(images), 0 if images is None else images.nbytes, C.byref(count))
    tm = np.ascontiguousarray(tiles if tiles is not None else [], dtype=np.uint64)
    if len(tm) and earliest is not None:
        place = np.ascontiguousarray(earliest, dtype=np.int32)
        if len(place) != len(nq):
            raise ValueError("one earliest pass per op expected")
        return lib.qsim_plan_ops_placed(*head, len(tm), ptr(tm), ptr(place), *tail), count.value
    rc = lib.qsim_plan_ops_tiled(*head, len(tm), ptr(tm), *tail) if len(tm) else lib.qsim_plan_ops(*head, *tail)
    return rc, count.value


def plan_ops(n: int, ops, tiles=None, earliest=None) -> np.ndarray:
    """The pass images (PASS_IMAGE) of the fused plan of `ops` on n qubits; `tiles`: uint64 masks, the high tile bits of
    the first passes named by the caller (qsim_plan_ops_tiled); `earliest`: with tiles, the placement of `balance` (op i
    not before pass earliest[i]: qsim_plan_ops_placed).  Planned once when the plan has up to 64 passes: the
    library fills the buffer it is given and fails at the first image that does not fit, the count then being the images
    written -- a full buffer is planned again into one of twice the size."""
    room = _FIRST_BUFFER
    while True:
        images = np.zeros(room, dtype=PASS_IMAGE)
        rc, count = _plan(n, ops, tiles, images, earliest)
        if rc != _lib.QSIM_ERR_INVALID or count < room:     # (any other failure leaves the buffer short of full, or shows again below)
            _lib.check(rc)
            return images[:count]
        room *= 2


def lower_images(images) -> tuple:
    """(the images as the device gets them, records rewritten): qsim_lower_pass_images on a copy of planned images -- the
    unconditional real 2x2 records of the unit-diagonal family as OPC_UNIT1, their factors folded into the pass."""
    out = np.ascontiguousarray(images, dtype=PASS_IMAGE).copy()
    count = C.c_int32()
    _lib.check(_lib.load().qsim_lower_pass_images(ptr(out), len(out), C.byref(count)))
    return out, count.value


def pass_count(n: int, ops, tiles=None, earliest=None) -> int:
    """len(plan_ops(n, ops, tiles, earliest)) without the images."""
    rc, count = _plan(n, ops, tiles, None, earliest)
    _lib.check(rc)
    return count


def balance(n: int, ops, tiles, pass_memory_us, engine_costs, place: bool = True) -> tuple:
    """(earliest, engine_us_before, engine_us_after) of qsim_plan_balance: the placement of `ops` over the passes named by
    `tiles` under pass time = max(pass_memory_us[p], engine time of the records priced by `engine_costs`) -- an op that
    needs no tile leaves a pass whose records cost more than its memory time for the pass with the most slack among those
    it may run in (up to the earliest pass of a later op that targets one of its qubits).  earliest: int32 per op (all zero
    when no placement is modelled cheaper), for `plan_ops` / `DeviceChunk.apply_ops_placed`; the other two: modelled engine
    microseconds per pass.  place = False: the passes are only priced (earliest is None, after = before)."""
    nq, qubits, mats = as_packed(ops)
    tm = np.ascontiguousarray(tiles, dtype=np.uint64)
    mem = np.ascontiguousarray(pass_memory_us, dtype=np.float64)
    costs = np.ascontiguousarray(engine_costs, dtype=np.float64)
    if len(mem) != len(tm):
        raise ValueError("one memory time per named pass expected")
    earliest = np.zeros(len(nq), dtype=np.int32) if place else None
    before, after = np.zeros(len(tm)), np.zeros(len(tm))
    _lib.check(_lib.load().qsim_plan_balance(n, len(nq), ptr(nq), ptr(qubits), ptr(mats), len(tm), ptr(tm), ptr(mem), ptr(costs),
                                             len(costs), ptr(earliest), ptr(before), ptr(after)))
    return earliest, before, after


def tiles_per_workgroup(n: int, tile_bits: int, fixed_bits: int = 0) -> int:
    """Tiles one workgroup of a fused pass takes on a chunk of n qubits (qsim_tiles_per_workgroup: the rule the launch
    itself applies, a pure function): 1, or 2 from 2 x 4096 tiles on; `fixed_bits`: those a partial launch of the split
    form fixes.  What the launch would refuse raises ValueError."""
    rc = int(_lib.load().qsim_tiles_per_workgroup(int(n), int(tile_bits), int(fixed_bits)))
    if rc < 0:
        _lib.check(rc)
    return rc


def search_tiles(n: int, ops, beam: int = 0) -> np.ndarray:
    """The tiles (one uint64 mask of high tile bits per pass) of the library's searching pass builder (qsim_plan_search:
    a beam search over the passes' tiles, `beam` 0 = its default width; never more passes than `plan_ops` makes)."""
    nq, qubits, mats = as_packed(ops)
    count = C.c_int32()
    out = np.zeros(len(nq), dtype=np.uint64)
    _lib.check(_lib.load().qsim_plan_search(n, len(nq), ptr(nq), ptr(qubits), ptr(mats), beam, ptr(out), len(out), C.byref(count)))
    return out[:count.value].copy()


HISTOGRAM_BINS = 64                # QSIM_PLAN_HISTOGRAM_BINS (include/qsim_hip.h)
TRIPLES_UNBOUNDED, TRIPLES_NEED_BITS = 1, 2     # QSIM_TRIPLES_* flags
_MASK_ROOM = 1 << 22               # most masks `search_triples` makes room for (32 MiB)


def search_triples(n: int, ops, triples=None, beam: int = 0, threads: int = 1, flags: int = 0) -> dict:
    """`search_tiles` of ONE op list under many line-qubit triples in one library call (qsim_plan_search_triples):
    `triples` is an int array of shape (m, 3), row t = the logical qubits that go to index bits 0, 1, 2 (the qubits that
    were there take their places: the candidate layouts of runner/layout_search.py); None = every a < b < c.  `threads`
    host threads share the fewest passes found so far, which ends the searches that cannot reach it -- the result is that
    of `search_tiles` triple by triple, whatever `threads` (TRIPLES_UNBOUNDED in `flags`: no search is ended).  Returns
    `passes` (the fewest), `index` / `triples` / `masks` (of every triple that reaches them, sorted by its qubits:
    position in `triples`, the three qubits, one uint64 mask per pass on the triple's index bits), `searched` (triples)
    and `histogram` ({passes: triples}; the triples above the fewest under the key None unless unbounded)."""
    nq, qubits, mats = as_packed(ops)
    tri = None if triples is None else np.ascontiguousarray(triples, dtype=np.int32).reshape(-1, 3)
    if tri is not None and not len(tri):
        raise ValueError("an empty list of triples (None searches them all)")
    m = n * (n - 1) * (n - 2) // 6 if tri is None else len(tri)
    best, count = C.c_int32(), C.c_int32()
    index, found = np.zeros(m, dtype=np.int32), np.zeros((m, 3), dtype=np.int32)
    room = min(_MASK_ROOM, m * max(1, len(nq)))
    masks, hist = np.zeros(room, dtype=np.uint64), np.zeros(HISTOGRAM_BINS, dtype=np.int32)
    _lib.check(_lib.load().qsim_plan_search_triples(n, len(nq), ptr(nq), ptr(qubits), ptr(mats), 0 if tri is None else m, ptr(tri),
                                                    beam, threads, flags, C.byref(best), C.byref(count), ptr(index), ptr(found),
                                                    ptr(masks), room, ptr(hist)))
    k, p = count.value, best.value
    histogram = {int(b): int(c) for b, c in enumerate(hist[:-1]) if c}
    if hist[-1]:
        histogram[None] = int(hist[-1])
    return {"passes": p, "index": index[:k].copy(), "triples": found[:k].copy(), "masks": masks[:k * p].reshape(k, p).copy(),
            "searched": m, "histogram": histogram}


def search_cycle(n: int, ops, triples, plain_passes=None, beam: int = 0, threads: int = 1) -> list:
    """Cyclic plans of ONE op list L that runs again and again, under the line-qubit triples given (qsim_plan_search_cycle):
    L.L is searched under every triple, L is cut at the first pass of that plan which holds an op of the second copy into a
    head A and a tail B, and A, B.A and B are searched under the same triple -- R executions are A (B.A)^(R-1) B
    (`device.Cycle`).  `plain_passes`: the passes of L under every triple, where known (else searched here).  Returns one
    dict per triple with the fewest steady passes, if those are fewer than its plain passes (an empty list: no cycle):
    `index` (position in `triples`), `triple`, `plain` / `head` / `steady` / `tail` (pass counts), `is_tail` (bool per op
    of L: it belongs to B; inside A and B the ops keep the order of L) and `masks` (three uint64 arrays: the tiles of A,
    B.A and B on the triple's index bits)."""
    nq, qubits, mats = as_packed(ops)
    tri = np.ascontiguousarray(triples, dtype=np.int32).reshape(-1, 3)
    m = len(tri)
    if not m:
        raise ValueError("an empty list of triples")
    plain = None if plain_passes is None else np.ascontiguousarray(plain_passes, dtype=np.int32)
    if plain is not None and len(plain) != m:
        raise ValueError("one plain pass count per triple expected")
    count = C.c_int32()
    index, found, passes = np.zeros(m, dtype=np.int32), np.zeros((m, 3), dtype=np.int32), np.zeros((m, 4), dtype=np.int32)
    tail = np.zeros((m, max(1, len(nq))), dtype=np.uint8)
    room = min(_MASK_ROOM, 3 * m * max(1, len(nq)))
    masks = np.zeros(room, dtype=np.uint64)
    _lib.check(_lib.load().qsim_plan_search_cycle(n, len(nq), ptr(nq), ptr(qubits), ptr(mats), m, ptr(tri), ptr(plain), beam, threads,
                                                  C.byref(count), ptr(index), ptr(found), ptr(passes), ptr(tail), ptr(masks), room))
    out, at = [], 0
    for f in range(count.value):
        cuts = at + np.concatenate([[0], np.cumsum(passes[f, 1:])])
        out.append({"index": int(index[f]), "triple": [int(q) for q in found[f]], "plain": int(passes[f, 0]), "head": int(passes[f, 1]),
                    "steady": int(passes[f, 2]), "tail": int(passes[f, 3]), "is_tail": tail[f, :len(nq)].astype(bool),
                    "masks": [masks[cuts[w]:cuts[w + 1]].copy() for w in range(3)]})
        at = int(cuts[3])
    return out


def rewrite_ops(n: int, ops, stats: dict = None, engine_costs=None) -> list:
    """`ops` rewritten for planning (qsim_rewrite_ops, csrc/op_rewrite.h): X / Y gates pushed into their neighbours, CNOTs
    with an exact H on the target turned into CZ -- the same amplitudes from fewer ops that need their target inside a
    tile.  `engine_costs` (the table of `runner.engine_cost.table()`, QSIM_ENGINE_COST_* entries) adds rule (d): diagonal
    1q gates multiplied into dense 1q gates where the table prices the product's record lower; None: pricing off.
    Returns [(qubits, U), ...]; `stats`, when given, receives ops_in, ops_out, need_tile_in, need_tile_out."""
    nq, qubits, mats = as_packed(ops)
    room = 2 * len(nq) + n
    out_nq, out_q = np.zeros(room, dtype=np.int32), np.zeros(2 * room, dtype=np.int32)
    out_m = np.zeros((room, 16), dtype=np.complex128)
    count, need = C.c_int32(), np.zeros(2, dtype=np.int32)
    costs = None if engine_costs is None else np.ascontiguousarray(engine_costs, dtype=np.float64)
    _lib.check(_lib.load().qsim_rewrite_ops_priced(n, len(nq), ptr(nq), ptr(qubits), ptr(mats), ptr(out_nq), ptr(out_q), ptr(out_m),
                                                   room, C.byref(count), ptr(need), ptr(costs), 0 if costs is None else len(costs)))
    if stats is not None:
        stats.update(ops_in=len(nq), ops_out=int(count.value), need_tile_in=int(need[0]), need_tile_out=int(need[1]))
    return [([int(out_q[2 * i])], out_m[i, :4].reshape(2, 2).copy()) if out_nq[i] == 1 else
            ([int(out_q[2 * i]), int(out_q[2 * i + 1])], out_m[i].reshape(4, 4).copy()) for i in range(count.value)]


def count_layouts(n: int, ops, layouts, threads: int) -> np.ndarray:
    """Passes of ONE op list under each layout (rows of `layouts`: qubit -> index bit), planned by `threads` threads of
    the library (qsim_plan_count_layouts): int32, one per row."""
    nq, qubits, mats = as_packed(ops)
    lay = np.ascontiguousarray(layouts, dtype=np.int32)
    out = np.zeros(len(lay), dtype=np.int32)
    _lib.check(_lib.load().qsim_plan_count_layouts(n, len(nq), ptr(nq), ptr(qubits), ptr(mats), len(lay), ptr(lay), ptr(out), threads))
    return out


def peek_pass(k: int, n: int, nq, qubits, mats, done, members, avoid: int = 0, hint: int = 0) -> tuple:
    """(tile mask, needed bits, member op indices) of the NEXT pass of a partly executed op list on a partitioned state
    (qsim_plan_peek_pass: index bits >= k of the n are rank bits; done[i] != 0: op i ran; `avoid`: bits the fill leaves
    out; `hint` != 0 names the tile).  The arrays are handed over as they are -- packed int32 / complex128, `done` uint8,
    `members` an int32 scratch of len(nq) or more -- because the partition planner asks thousands of times per schedule."""
    mask, need, count = C.c_uint64(), C.c_uint64(), C.c_int32()
    _lib.check(_lib.load().qsim_plan_peek_pass(k, n, len(nq), ptr(nq), ptr(qubits), ptr(mats), ptr(done), avoid, hint,
                                               C.byref(mask), C.byref(need), C.byref(count), ptr(members)))
    return int(mask.value), int(need.value), [int(i) for i in members[:count.value]]


def plan_pauli_rotations(n: int, x_masks) -> tuple:
    """The pass plan of `DeviceChunk.apply_pauli_rotations` on a chunk of n qubits (qsim_plan_pauli_rotations, device-free):
    (pass of every rotation, tile-bit mask of every pass; 0 = a wide pass of one rotation).  Order preserving -- rotations
    exp(-i theta P) do not commute -- so the passes are runs of the list and `pass_of` never decreases."""
    x = np.ascontiguousarray(x_masks, dtype=np.uint64).reshape(-1)
    pass_of = np.empty(x.size, dtype=np.int32)
    tiles = np.empty(max(x.size, 1), dtype=np.uint64)
    count = C.c_int(0)
    _lib.check(_lib.load().qsim_plan_pauli_rotations(int(n), int(x.size), ptr(x), ptr(pass_of), ptr(tiles), C.byref(count)))
    return pass_of, tiles[:count.value].copy()
