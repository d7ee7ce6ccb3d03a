"""Cyclic plans on the CPU (csrc/tile_search.h plan_search_cycle, `qsim_plan_search_cycle`, `planner.search_cycle`): an op
list L that runs again and again is cut into a head A and a tail B, and R executions run as A (B.A)^(R-1) B.  Structure of
what the search returns (A and B partition L, the three tile lists replay into the counts, the result does not depend on
the thread count), meaning (the pass images of head, steady x 2, tail, walked by tests/tile_interpreter.py, give the dense
oracle's L.L.L to 1e-12 -- for hand-made cycles, whose tail is the last m ops of L, and for returned ones), and the bench
list (28 qubits: a cycle with fewer steady passes than the plain 13 is found).  No device."""
import functools
import itertools

import numpy as np
import pytest

from oracle import dense_oracle as orc
from quantum_simulations_amd.kernel import planner
from quantum_simulations_amd.runner import layout_search
from tests import tile_interpreter
from tests.test_plan_triples_cpu import SIZES, _ops, _relabelled

ATOL = 1e-12


def _triples(n):
    return np.array(list(itertools.combinations(range(n), 3)), dtype=np.int32)


@functools.lru_cache(maxsize=None)
def _cycles(n, threads=4):
    return planner.search_cycle(n, _ops(n), _triples(n), None, 0, threads)


def _parts(ops, is_tail):
    head = [op for op, late in zip(ops, is_tail) if not late]
    tail = [op for op, late in zip(ops, is_tail) if late]
    return head, tail + head, tail


def _rand_state(n, seed):
    rng = np.random.default_rng(seed)
    psi = rng.normal(size=1 << n) + 1j * rng.normal(size=1 << n)
    return psi / np.linalg.norm(psi)


@functools.lru_cache(maxsize=None)
def _thrice(n):
    """(a random state, the dense oracle's L.L.L of it): computed once per size"""
    psi0 = _rand_state(n, 100 + n)
    want = psi0.copy()
    for _ in range(3):
        orc.apply_ops(want, _ops(n))
    psi0.setflags(write=False)
    want.setflags(write=False)
    return psi0, want


def _walk(n, psi0, lists, tiles=(None, None, None)):
    """head, steady, steady, tail through the tile interpreter"""
    psi = np.array(psi0)
    images = [planner.plan_ops(n, ops, ms) for ops, ms in zip(lists, tiles)]
    for which in (0, 1, 1, 2):
        tile_interpreter.run(psi, images[which])
    return psi, [len(i) for i in images]


@pytest.mark.parametrize("n", SIZES)
def test_what_the_search_returns_is_a_partition_that_replays(n):
    ops, triples = _ops(n), _triples(n)
    layouts = layout_search.triple_layouts(n, triples)
    cycles = _cycles(n)
    print(f"n = {n}: {len(ops)} ops, {len(triples)} triples, {len(cycles)} cycles "
          f"{[(c['triple'], c['plain'], c['head'], c['steady'], c['tail']) for c in cycles[:4]]}")
    for c in cycles:
        assert c["triple"] == triples[c["index"]].tolist()
        assert len(c["is_tail"]) == len(ops) and c["is_tail"].any() and not c["is_tail"].all()
        assert c["steady"] < c["plain"] and c["steady"] == cycles[0]["steady"]
        moved = _relabelled(ops, layouts[c["index"]])
        assert c["plain"] == len(planner.search_tiles(n, moved))
        for part, masks, count in zip(_parts(moved, c["is_tail"]), c["masks"], (c["head"], c["steady"], c["tail"])):
            assert len(masks) == count and planner.pass_count(n, part, masks) == count


@pytest.mark.parametrize("n", SIZES)
def test_the_result_does_not_depend_on_the_thread_count(n):
    want = _cycles(n)
    for threads in (1, 3, 16):
        got = planner.search_cycle(n, _ops(n), _triples(n), None, 0, threads)
        assert len(got) == len(want), threads
        for a, b in zip(got, want):
            assert all(np.array_equal(a[key], b[key]) for key in ("index", "triple", "plain", "head", "steady", "tail", "is_tail")), threads
            assert all(np.array_equal(x, y) for x, y in zip(a["masks"], b["masks"])), threads


def test_known_plain_passes_give_the_same_cycles():
    n = SIZES[-1]
    ops, triples = _ops(n), _triples(n)
    res = planner.search_triples(n, ops, triples, 0, 4)
    got = planner.search_cycle(n, ops, res["triples"], [res["passes"]] * len(res["triples"]), 0, 4)
    for c in got:
        assert c["plain"] == res["passes"] and c["steady"] < res["passes"]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("share", ("one", "tenth", "half"))
def test_a_hand_made_cycle_walks_into_three_executions(n, share):
    """the last m ops of L as the tail: a product of L whatever m is"""
    ops = _ops(n)
    m = {"one": 1, "tenth": max(2, len(ops) // 10), "half": len(ops) // 2}[share]
    is_tail = np.arange(len(ops)) >= len(ops) - m
    psi0, want = _thrice(n)
    got, passes = _walk(n, psi0, _parts(ops, is_tail))
    err = float(np.max(np.abs(got - want)))
    print(f"n = {n}, tail of {m} of {len(ops)} ops: passes head / steady / tail {passes}, max |walk - oracle| {err:.3e}")
    assert err <= ATOL


@pytest.mark.parametrize("n", SIZES)
def test_a_returned_cycle_walks_into_three_executions(n):
    ops, triples = _ops(n), _triples(n)
    layouts = layout_search.triple_layouts(n, triples)
    for c in _cycles(n)[:3]:
        moved = _relabelled(ops, layouts[c["index"]])
        psi0 = _rand_state(n, 7)
        want = psi0.copy()
        for _ in range(3):
            orc.apply_ops(want, moved)
        got, passes = _walk(n, psi0, _parts(moved, c["is_tail"]), c["masks"])
        err = float(np.max(np.abs(got - want)))
        print(f"n = {n}, triple {c['triple']}: passes {passes} (plain {c['plain']}), max |walk - oracle| {err:.3e}")
        assert passes == [c["head"], c["steady"], c["tail"]] and err <= ATOL


def test_no_triple_with_a_cycle_is_a_result():
    """two ops on one qubit: one pass whatever is done, so nothing can be saved"""
    ops = [([3], np.array([[0, 1], [1, 0]], dtype=complex) @ np.diag([1, 1j])), ([3], np.diag([1, 1j]))]
    assert planner.search_cycle(12, ops, [[0, 1, 2]], None, 0, 2) == []


def test_the_bench_list_has_a_cycle_below_its_plain_passes():
    from quantum_simulations_amd.circuit.fusion import batch_levels
    from quantum_simulations_amd.circuit.io import levelize, validate_circuit_dict
    from quantum_simulations_amd.circuits import random_1q_cx_circuit
    n = 28
    cd = validate_circuit_dict(random_1q_cx_circuit(n, depth=40))
    (own,) = [p["local_ops"] for p in batch_levels(levelize(cd), n)]
    ops = planner.rewrite_ops(n, own)
    triples = np.array([[7, 5, 20], [19, 22, 27], [27, 15, 25], [2, 11, 9]], dtype=np.int32)
    cycles = planner.search_cycle(n, ops, triples, None, 0, 8)
    print(f"{len(ops)} ops: {[(c['triple'], c['plain'], c['head'], c['steady'], c['tail']) for c in cycles]}")
    assert cycles and all(c["plain"] == 13 and c["steady"] < 13 for c in cycles)
    layouts = layout_search.triple_layouts(n, triples)
    for c in cycles:
        moved = _relabelled(ops, layouts[c["index"]])
        for part, masks, count in zip(_parts(moved, c["is_tail"]), c["masks"], (c["head"], c["steady"], c["tail"])):
            assert planner.pass_count(n, part, masks) == count
