"""The layout search of a single-GPU plan, on the host only: which index bit every logical qubit lives on
(`choose_plan_layout`, with `priced_variant` and `pass_memory_us`), and the SWAPs between two layouts (`layout_swaps`).
`runner/engine.py` plans with these (`SingleGpuEngine.plan_batches`) and imports their names: callers find them there too."""
from __future__ import annotations

import numpy as np

from quantum_simulations_amd.kernel import planner


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


PLACED_PER_FINALIST = 4            # minimum-pass layouts placed and priced for every finalist `choose_plan_layout` returns
CYCLE_FINALISTS = 4                # cyclic plans (`planner.search_cycle`) placed and priced next to the plain finalists, at most
CYCLE_STEADY_WEIGHT = 8            # most copies of the steady tiles the placement of a cyclic plan sets against one of its head and tail tiles


def candidate_triples(n: int, n_candidates: int, seed: int) -> np.ndarray:
    """The line-qubit triples `choose_plan_layout` searches, int32 (n_candidates + 1, 3): the identity (0, 1, 2), then
    n_candidates random ones from one generator, so a longer list starts with the shorter one."""
    rng = np.random.default_rng(seed)
    rows = [[0, 1, 2]] + [[int(x) for x in rng.choice(n, size=3, replace=False)] for _ in range(n_candidates)]
    return np.array(rows, dtype=np.int32)


def triple_layouts(n: int, triples) -> np.ndarray:
    """Rows qubit -> index bit, one per triple: from the identity, the qubit on line bit b trades places with triple[b]
    (the rule of the library's triple_layout, csrc/tile_search.h)."""
    layouts = np.tile(np.arange(n, dtype=np.int32), (len(triples), 1))
    for row, triple in zip(layouts, triples):
        for bit, q in enumerate(int(x) for x in triple):
            j = int(np.flatnonzero(row == bit)[0])          # the qubit on `bit` trades places with q
            row[j], row[q] = row[q], bit
    return layouts


def _search_triples(n: int, batches, triples, layouts, beam: int, threads: int) -> tuple:
    """(fewest passes of the batches over the triples, {candidate: tile masks per batch} of the candidates that reach them,
    {passes: candidates}).  One op list of two ops or more: one library call, whose searches share their bound
    (`planner.search_triples`; candidates above the fewest are counted under ">fewest").  Several: the sum over the lists
    decides, which no bound on one of them knows, so every list is searched to the end under every triple."""
    none = np.zeros(0, dtype=np.uint64)
    short = sum(len(ops) for ops in batches if len(ops) < 2)                    # (a single op is not searched: one pass)
    long = [i for i, ops in enumerate(batches) if len(ops) >= 2]
    if len(long) == 1:
        res = planner.search_triples(n, batches[long[0]], triples, beam, threads)
        best = short + res["passes"]
        found = {int(t): [ms if i == long[0] else none for i in range(len(batches))] for t, ms in zip(res["index"], res["masks"])}
        by_passes = {best: len(found)}
        if len(found) < len(triples):
            by_passes[f">{best}"] = len(triples) - len(found)
        return best, found, by_passes
    from concurrent.futures import ThreadPoolExecutor

    def search(lay):                                        # (the library call releases the interpreter lock)
        return [planner.search_tiles(n, [([int(lay[q]) for q in qs], U) for qs, U in ops], beam) if len(ops) >= 2 else none
                for ops in batches]
    with ThreadPoolExecutor(threads) as pool:
        every = list(pool.map(search, layouts))
    counts = np.array([short + sum(len(ms) for ms in f) for f in every], dtype=np.int64)
    best = int(counts.min())
    return (best, {int(t): every[t] for t in np.flatnonzero(counts == best)},
            {int(c): int((counts == c).sum()) for c in np.unique(counts)})


def choose_plan_layout(n: int, batches, n_candidates: int = 31, seed: int = 20260504, n_finalists: int = 4,
                       all_finalists: bool = False, beam: int = 0, engine_costs=None, priced_batches=None, cycle_repeats: int = 0):
    """(l2p, tile masks per batch on the chosen index bits, info) for the op lists `batches` (logical qubits).  The three
    qubits on the line bits belong to every tile, so they decide how many passes a plan needs; which index bits the OTHER
    qubits live on does not (a relabelling of the bits >= 3 maps every valid pass sequence to a valid one).  So: for the
    identity and `n_candidates` random line-qubit triples (`candidate_triples`) the library's searching pass builder
    plans the batches in one call (qsim_plan_search_triples, beam width `beam`, 0 = its default; `_search_triples`); of
    the triples that need the fewest passes the first PLACED_PER_FINALIST * n_finalists are kept and their other qubits
    placed by the tile-cost model (runner/tile_layout.py), on a thread pool.  Host only.  all_finalists: the list of the
    n_finalists of those that the model prices lowest, best first (the engine may time them on the device).  info:
    `candidates_by_passes` ({passes: candidates}; one op list: the fewest and ">fewest"), `minimum_pass_triples` (how many
    candidates reach the fewest passes), `line_qubits` (the layout's triple).
    engine_costs (the table of runner/engine_cost.py; None: pricing off): a pass is priced max(memory model of its tile,
    engine time of its records); `priced_variant` then chooses between `batches` and `priced_batches` (the same lists
    under rule (d) of the rewrite, optional) and places the ops that need no tile: info gains `planned` (the op lists to
    run, on their index bits), `placed` (their placements, per batch) and the modelled split (`model_split_ms`), and the
    finalists rank by that total instead of the memory model alone.
    cycle_repeats > 0 (one op list, all_finalists): the plan is made for that many executions one after the other, and the
    cyclic plans of the list under its minimum-pass triples (`planner.search_cycle`: the tail of one execution runs with
    the head of the next, a pass fewer per execution where one is found) join the finalists, after n_finalists plain ones.
    One layout serves the three lists of a cycle: its other qubits are placed over the steady tiles, min(cycle_repeats,
    CYCLE_STEADY_WEIGHT) times each, and the head and tail tiles once; pricing applies to each list as to one list; the
    model total is that of the steady passes.  info["cycle"]: `planned`, `tiles`, `placed` (three each: head, steady,
    tail), `passes` (the three counts) and `plain_passes`."""
    import os

    from quantum_simulations_amd import _lib
    from quantum_simulations_amd.runner import tile_layout
    triples = candidate_triples(n, n_candidates, seed)
    layouts = triple_layouts(n, triples)
    try:
        threads = len(os.sched_getaffinity(0))
    except AttributeError:
        threads = os.cpu_count() or 1
    threads = max(1, min(16, threads))
    _lib.load()

    def relabelled(lay):
        return [[([int(lay[q]) for q in qs], U) for qs, U in ops] for ops in batches]
    best, found, by_passes = _search_triples(n, batches, triples, layouts, beam, threads)
    # The layouts to place and price: minimum-pass candidates in candidate order (the identity first when it ties),
    # PLACED_PER_FINALIST of them for every finalist asked for.  The finalists are the lowest of those by the model, which
    # separates good from bad layouts though it does not rank the best.
    tried = sorted(found)[:PLACED_PER_FINALIST * max(1, n_finalists)]
    greedy_identity = int(_count_passes(n, batches, layouts[:1], 1)[0])
    from concurrent.futures import ThreadPoolExecutor
    tile_layout.model_for(n)                                    # (loaded before the threads ask for it)

    def annealed(job):                                          # (the library call releases the interpreter lock)
        f, s = job
        return tile_layout.choose_layout([[b for b in range(tile_layout.LOW, n) if (int(m) >> b) & 1] for ms in found[f] for m in ms], n, seed=s)
    with ThreadPoolExecutor(threads) as pool:                   # eight annealing runs per layout, all layouts at once
        runs = list(pool.map(annealed, [(f, s) for f in tried for s in range(1, 9)]))

    def placed(at):
        f = tried[at]
        first = [int(x) for x in layouts[f]]
        moved = relabelled(first)
        masks = found[f]
        second, cost0, cost1 = min(runs[8 * at:8 * at + 8], key=lambda r: r[2])
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
                "candidates_by_passes": dict(by_passes), "minimum_pass_triples": len(found), "line_qubits": [int(q) for q in triples[f]],
                "beam": int(beam) if beam > 0 else "default",
                "model_ms": (round(cost0, 3), round(cost1, 3))}
        if engine_costs is not None:
            def on_bits(lists):
                return [[([l2p[q] for q in qs], U) for qs, U in ops] for ops in lists]
            # info["planned"]: the op lists the plan runs (on their index bits), info["placed"]: their placements
            info["planned"], info["placed"], info["model_split_ms"] = priced_variant(
                n, on_bits(batches), None if priced_batches is None else on_bits(priced_batches), final_masks, engine_costs)
            info["passes_chosen"] = info["model_split_ms"]["pass_count"]       # (a list under rule (d) may finish a pass early)
        return l2p, final_masks, info
    def modelled(r):
        return r[2]["model_split_ms"]["passes"] if "model_split_ms" in r[2] else r[2]["model_ms"][1]

    def cycle_tiles(c):                                         # (the steady tiles weigh `cycle_repeats` to one, up to the cap)
        weights = [1, max(1, min(int(cycle_repeats), CYCLE_STEADY_WEIGHT)), 1]
        return [[b for b in range(tile_layout.LOW, n) if (int(m) >> b) & 1] for ms, w in zip(c["masks"], weights) for m in list(ms) * w]

    def cyclic(job):
        c, annealings = job
        f = sorted(found)[c["index"]]
        first = [int(x) for x in layouts[f]]
        ops = batches[0]
        head = [op for op, late in zip(ops, c["is_tail"]) if not late]
        tail = [op for op, late in zip(ops, c["is_tail"]) if late]
        parts, counts = [head, tail + head, tail], [c["head"], c["steady"], c["tail"]]
        second = min(annealings, key=lambda r: r[2])[0]

        def moved(lists, lay):
            return [[([lay[first[q]] for q in qs], U) for qs, U in part] for part in lists]

        def on_bits(lay):
            return [np.array([sum(1 << lay[b] for b in range(n) if (int(m) >> b) & 1) for m in ms], dtype=np.uint64) for ms in c["masks"]]
        masks = on_bits(second)
        # (as for a plain plan: a placement under which a list would replay into other passes is dropped for the searched one)
        if [planner.pass_count(n, part, ms) for part, ms in zip(moved(parts, second), masks)] != counts:
            second = list(range(n))
            masks = on_bits(second)
        l2p = [second[first[q]] for q in range(n)]
        info = {"passes_identity": greedy_identity, "passes_chosen": c["steady"], "candidates": n_candidates + 1,
                "candidates_by_passes": dict(by_passes), "minimum_pass_triples": len(found), "line_qubits": [int(q) for q in triples[f]],
                "beam": int(beam) if beam > 0 else "default",
                # (of the steady passes alone: what the annealing priced holds their copies and the head and tail tiles too)
                "model_ms": tuple(round(float(pass_memory_us(n, ms).sum()) / 1e3, 3) for ms in (on_bits(list(range(n)))[1], masks[1]))}
        planned, places = moved(parts, second), [None, None, None]
        if engine_costs is not None:
            for w in range(3):
                priced = planner.rewrite_ops(n, planned[w], None, engine_costs)
                (planned[w],), (places[w],), split = priced_variant(n, [planned[w]], [priced], [masks[w]], engine_costs)
                counts[w] = split["pass_count"]
                if w == 1:
                    info["model_split_ms"] = split
            info["passes_chosen"] = counts[1]
        info["cycle"] = {"planned": planned, "tiles": masks, "placed": places, "passes": [int(x) for x in counts], "plain_passes": int(c["plain"])}
        return l2p, [masks[1]], info
    with ThreadPoolExecutor(threads) as pool:
        out = list(pool.map(placed, range(len(tried))))
        out.sort(key=modelled)
        out = out[:max(1, n_finalists)]
        if cycle_repeats > 0 and all_finalists and len(batches) == 1 and len(batches[0]) >= 2:
            plain = [best] * len(found)
            cycles = planner.search_cycle(n, batches[0], triples[sorted(found)], plain, beam, threads)[:CYCLE_FINALISTS]
            anneal = list(pool.map(lambda job: tile_layout.choose_layout(cycle_tiles(job[0]), n, seed=job[1]),
                                   [(c, s) for c in cycles for s in range(1, 9)]))
            out += list(pool.map(cyclic, [(c, anneal[8 * i:8 * i + 8]) for i, c in enumerate(cycles)]))
            out.sort(key=modelled)
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
