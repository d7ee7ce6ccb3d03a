"""The line-qubit triple search on the CPU (csrc/tile_search.h plan_search_triples, `qsim_plan_search_triples`,
`planner.search_triples`): one library call over many triples, with a bound shared between its threads, returns what
`planner.search_tiles` returns triple by triple -- the fewest passes, the triples that reach them, their tiles -- whatever
the thread count; and `choose_plan_layout`, which calls it once, over the candidates it searched before.  No device."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

from quantum_simulations_amd import _lib
from quantum_simulations_amd._lib import ptr
from quantum_simulations_amd.kernel import planner
from quantum_simulations_amd.kernel.device import pack_ops
from quantum_simulations_amd.runner import layout_search

SIZES = (12, 14)


@functools.lru_cache(maxsize=None)
def _ops(n, depth=40):
    from quantum_simulations_amd.circuit.io import validate_circuit_dict
    from quantum_simulations_amd.circuits import random_1q_cx_circuit
    from quantum_simulations_amd.runner.engine import gate_ops
    return planner.rewrite_ops(n, gate_ops(validate_circuit_dict(random_1q_cx_circuit(n, depth=depth, seed=n))))


def _relabelled(ops, lay):
    return [([int(lay[q]) for q in qs], U) for qs, U in ops]


@functools.lru_cache(maxsize=None)
def _one_by_one(n):
    """(all triples ascending, their layouts, the tiles `search_tiles` finds under each): the reference, computed once"""
    triples = np.array(list(itertools.combinations(range(n), 3)), dtype=np.int32)
    layouts = layout_search.triple_layouts(n, triples)
    return triples, layouts, [planner.search_tiles(n, _relabelled(_ops(n), lay)) for lay in layouts]


def _same(a, b):
    return (a["passes"] == b["passes"] and np.array_equal(a["index"], b["index"]) and np.array_equal(a["triples"], b["triples"])
            and np.array_equal(a["masks"], b["masks"]) and a["searched"] == b["searched"])


@pytest.mark.parametrize("n", SIZES)
def test_all_triples_equal_the_searches_one_by_one(n):
    triples, layouts, tiles = _one_by_one(n)
    counts = np.array([len(ms) for ms in tiles])
    best = int(counts.min())
    res = planner.search_triples(n, _ops(n), None, 0, 4)
    print(f"n = {n}: {len(_ops(n))} ops, passes by triple {np.bincount(counts).tolist()}, histogram {res['histogram']}")
    assert res["passes"] == best and res["searched"] == len(triples)
    assert np.array_equal(res["index"], np.flatnonzero(counts == best))              # (ascending triples: sorted as they come)
    assert np.array_equal(res["triples"], triples[res["index"]])
    for t, masks in zip(res["index"], res["masks"]):
        assert np.array_equal(masks, tiles[t])
        assert planner.pass_count(n, _relabelled(_ops(n), layouts[t]), masks) == best     # the tiles replay into `best` passes
    assert res["histogram"][best] == len(res["index"])
    assert sum(res["histogram"].values()) == len(triples) and min(p for p in res["histogram"] if p is not None) == best
    # unbounded, every count is exact
    full = planner.search_triples(n, _ops(n), None, 0, 4, planner.TRIPLES_UNBOUNDED)
    assert _same(full, res) and full["histogram"] == {int(p): int(c) for p, c in enumerate(np.bincount(counts)) if c}


def test_the_bound_has_something_to_cut_at_14_qubits():
    counts = np.array([len(ms) for ms in _one_by_one(14)[2]])
    assert counts.min() >= 2 and (counts > counts.min()).any()


@pytest.mark.parametrize("n", SIZES)
def test_the_result_does_not_depend_on_threads_or_bound(n):
    want = planner.search_triples(n, _ops(n), None, 0, 1)
    for threads in (3, 16):
        for flags in (0, planner.TRIPLES_NEED_BITS, planner.TRIPLES_UNBOUNDED):
            assert _same(planner.search_triples(n, _ops(n), None, 0, threads, flags), want), (threads, flags)


def test_a_list_with_the_identity_first():
    """The identity triple is `search_tiles` of the list as it stands; the found triples come sorted by their qubits, with
    their positions in the caller's list, a repeated triple after its twin."""
    n = 14
    all_triples, layouts, tiles = _one_by_one(n)
    rng = np.random.default_rng(3)
    picks = [0] + [int(t) for t in rng.choice(len(all_triples), size=40, replace=False)]
    given = all_triples[picks + [picks[5]]]
    given[7] = given[7][::-1]                                   # (a descending triple: another layout, searched here)
    res = planner.search_triples(n, _ops(n), given, 0, 3)
    counts = np.array([len(tiles[t]) for t in picks + [picks[5]]])
    counts[7] = len(planner.search_tiles(n, _relabelled(_ops(n), layout_search.triple_layouts(n, given[7:8])[0])))
    best = int(counts.min())
    assert res["passes"] == best and sorted(res["index"]) == [int(i) for i in np.flatnonzero(counts == best)]
    keys = [tuple(int(q) for q in t) + (int(i),) for t, i in zip(res["triples"], res["index"])]
    assert keys == sorted(keys) and np.array_equal(res["triples"], given[res["index"]])
    alone = planner.search_triples(n, _ops(n), given[:1], 0, 1)
    assert alone["passes"] == len(tiles[0]) and np.array_equal(alone["masks"][0], planner.search_tiles(n, _ops(n)))
    assert alone["index"].tolist() == [0] and alone["triples"].tolist() == [[0, 1, 2]]


def test_fewer_than_two_ops():
    n = 12
    for ops in ([], _ops(n)[:1]):
        res = planner.search_triples(n, ops, [[0, 1, 2], [4, 9, 2]], 0, 2)
        assert res["passes"] == len(ops) and res["index"].tolist() == [0, 1] and res["masks"].shape == (2, len(ops))
        assert res["histogram"] == {len(ops): 2}


def test_bad_triples_and_buffers_are_refused():
    n = 12
    nq, qubits, mats = pack_ops(_ops(n))
    lib = _lib.load()
    best, count = C.c_int32(), C.c_int32()
    index, found, masks = np.zeros(2, dtype=np.int32), np.zeros(6, dtype=np.int32), np.zeros(2 * len(nq), dtype=np.uint64)

    def call(triples, room=len(masks), qubits_n=n):
        tri = np.ascontiguousarray(triples, dtype=np.int32)
        return lib.qsim_plan_search_triples(qubits_n, len(nq), ptr(nq), ptr(qubits), ptr(mats), len(tri), ptr(tri), 0, 2, 0,
                                            C.byref(best), C.byref(count), ptr(index), ptr(found), ptr(masks), room, None)
    assert call([[0, 1, 2], [5, 3, 5]]) == _lib.QSIM_ERR_INVALID            # a repeated qubit
    assert call([[7, 7, 2]]) == _lib.QSIM_ERR_INVALID
    assert call([[0, 1, n]]) == _lib.QSIM_ERR_INVALID                       # a qubit outside the register
    assert call([[0, 1, -1]]) == _lib.QSIM_ERR_INVALID
    assert call([[0, 1, 2]], qubits_n=4) == _lib.QSIM_ERR_INVALID           # below the fused-pass minimum
    assert call([[0, 1, 2], [5, 3, 4]], room=1) == _lib.QSIM_ERR_INVALID and best.value > 1 and count.value >= 1   # too small a buffer
    assert call([[0, 1, 2], [5, 3, 4]]) == _lib.QSIM_OK
    with pytest.raises(ValueError):
        planner.search_triples(n, _ops(n), [[1, 1, 2]])


def test_the_first_candidates_are_the_ones_searched_before():
    """identity + random triples from the same generator and seed: the layouts of the first 32 are those the search drew
    when it searched 32 (restated here as it was written then)."""
    n, seed = 26, 20260504
    rng = np.random.default_rng(seed)
    before = np.tile(np.arange(n, dtype=np.int32), (32, 1))
    for row in before[1:]:
        for bit, q in enumerate(int(x) for x in rng.choice(n, size=3, replace=False)):
            j = int(np.flatnonzero(row == bit)[0])
            row[j], row[q] = row[q], bit
    from quantum_simulations_amd.runner.engine import SingleGpuEngine
    assert SingleGpuEngine.LAYOUT_CANDIDATES >= 31
    triples = layout_search.candidate_triples(n, SingleGpuEngine.LAYOUT_CANDIDATES, seed)
    assert np.array_equal(layout_search.triple_layouts(n, triples)[:32], before)
    assert np.array_equal(triples[:32], layout_search.candidate_triples(n, 31, seed))


def test_choose_plan_layout_returns_minimum_pass_finalists():
    """LAYOUT_MIN_QUBITS qubits, depth 8, the engine's candidate count: every finalist needs `passes_chosen` passes, on its
    own line qubits."""
    from quantum_simulations_amd.circuit.io import validate_circuit_dict
    from quantum_simulations_amd.circuits import random_1q_cx_circuit
    from quantum_simulations_amd.runner.engine import SingleGpuEngine, gate_ops
    n = SingleGpuEngine.LAYOUT_MIN_QUBITS
    assert n == 26
    ops = planner.rewrite_ops(n, gate_ops(validate_circuit_dict(random_1q_cx_circuit(n, depth=8))))
    finalists = layout_search.choose_plan_layout(n, [ops], SingleGpuEngine.LAYOUT_CANDIDATES, n_finalists=SingleGpuEngine.LAYOUT_FINALISTS,
                                                 all_finalists=True)
    assert 1 <= len(finalists) <= SingleGpuEngine.LAYOUT_FINALISTS
    chosen = finalists[0][2]["passes_chosen"]
    costs = [info["model_ms"][1] for _, _, info in finalists]
    assert costs == sorted(costs)
    for l2p, masks, info in finalists:
        assert sorted(l2p) == list(range(n)) and info["passes_chosen"] == chosen
        assert info["candidates"] == SingleGpuEngine.LAYOUT_CANDIDATES + 1 == sum(info["candidates_by_passes"].values())
        assert info["candidates_by_passes"][chosen] == info["minimum_pass_triples"] >= len(finalists)
        assert sorted(l2p[q] for q in info["line_qubits"]) == [0, 1, 2]                  # its triple sits on the line bits
        assert planner.pass_count(n, _relabelled(ops, l2p), masks[0]) == chosen == len(masks[0])
    # no candidate the search dropped needs fewer passes: the identity and two more, one by one
    triples = layout_search.candidate_triples(n, SingleGpuEngine.LAYOUT_CANDIDATES, 20260504)
    for lay in layout_search.triple_layouts(n, triples[[0, 9, 20]]):
        assert len(planner.search_tiles(n, _relabelled(ops, lay))) >= chosen
