"""The searching pass builder on the CPU (csrc/tile_search.h, `qsim_plan_search`): the tiles it names replay through
`qsim_plan_ops_tiled` into correct passes (tests/tile_interpreter.py against the dense oracle), into exactly the number of
passes it reports, and never into more than the greedy builder needs.  No device involved."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import dense_oracle as orc
from quantum_simulations_amd import _lib
from quantum_simulations_amd._lib import ptr as _ptr
from quantum_simulations_amd.kernel import planner
from quantum_simulations_amd.kernel.device import pack_ops
from tests import tile_interpreter as ti
from tests.test_gpu_kernels import _rand_state, _random_ops


def search(n, ops, beam=0):
    """(reported pass count, tile masks) of the searching builder"""
    masks = planner.search_tiles(n, ops, beam)
    return len(masks), masks


def plan_tiled(n, ops, masks):
    """pass images of `ops` under the named tiles (qsim_plan_ops_tiled)"""
    return planner.plan_ops(n, ops, masks)


def _commuting_ops(n, seed, n_hubs=40):
    """Fans of CNOTs from one control / into one target, CZ / CR on a hub, X on targets, Z / S / T on controls: neighbours
    that commute across an op that has to wait (the blocking rules bt / bd / bx the two builders share)."""
    rng = np.random.default_rng(seed)
    CNOT, CZ = orc.gate_matrix("CNOT"), orc.gate_matrix("CZ")
    ops = []
    for _ in range(n_hubs):
        hub = int(rng.integers(n))
        others = [int(q) for q in rng.permutation(n) if q != hub][:int(rng.integers(2, 6))]
        kind = rng.random()
        for q in others:
            if kind < 0.35:
                ops.append(([hub, q], CNOT))                                   # common control
            elif kind < 0.7:
                ops.append(([q, hub], CNOT))                                   # common target
            elif kind < 0.85:
                ops.append(([hub, q], CZ if rng.random() < 0.5 else orc.gate_matrix("CR", {"k": int(rng.integers(2, 5))})))
            else:
                ops.append(([q, hub], orc.gate_matrix("CY")))                  # Y on the target: not X-type
            r = rng.random()
            if r < 0.25:
                ops.append(([hub], orc.gate_matrix("X" if 0.35 <= kind < 0.7 else "T")))
            elif r < 0.35:
                ops.append(([int(rng.integers(n))], orc.gate_matrix("H")))
    return ops


@functools.lru_cache(maxsize=None)
def _bench_ops(n):
    from quantum_simulations_amd.circuit.fusion import batch_levels
    from quantum_simulations_amd.circuit.io import levelize, validate_circuit_dict
    from quantum_simulations_amd.circuits import random_1q_cx_circuit
    batches = [p["local_ops"] for p in batch_levels(levelize(validate_circuit_dict(random_1q_cx_circuit(n, depth=40))), n)]
    assert len(batches) == 1
    return batches[0]


@functools.lru_cache(maxsize=None)
def _bench_search(n):
    return search(n, _bench_ops(n))


@pytest.mark.parametrize("n", [9, 11, 12, 14])
def test_searched_tiles_replay_into_correct_passes(n):
    """Random op lists and lists of commuting neighbours: the searched tiles, planned by qsim_plan_ops_tiled and executed by
    the interpreter, give the oracle's state; the replay has exactly the reported number of passes."""
    lists = [_random_ops(n, 120, 9100 + 10 * n + seed) for seed in range(3)] + [_commuting_ops(n, 9200 + 10 * n + seed) for seed in range(3)]
    for case, ops in enumerate(lists):
        count, masks = search(n, ops, beam=4)
        images = plan_tiled(n, ops, masks)
        assert len(images) == count == len(masks), (n, case)
        assert count <= len(ti.plan(n, ops)), (n, case)
        psi = _rand_state(n, 400 + case)
        want = psi.copy()
        orc.apply_ops(want, ops)
        ti.run(psi, images)
        np.testing.assert_allclose(psi, want, rtol=0, atol=1e-12, err_msg=f"n={n} case={case}")


def test_search_never_needs_more_passes_than_the_greedy_builder():
    """A few dozen seeded lists on 12..20 qubits (more qubits than a tile holds: there is a choice to make) and the two
    bench circuits: reported count <= greedy count, and the replay of the tiles has the reported count."""
    rng = np.random.default_rng(77)
    cases = []
    for seed in range(30):
        n = int(rng.integers(12, 21))
        cases.append((n, _random_ops(n, 150, 9300 + seed) if seed % 3 else _commuting_ops(n, 9300 + seed, 50)))
    better = 0
    for n, ops in cases:
        count, masks = search(n, ops, beam=4)
        greedy = len(ti.plan(n, ops))
        assert count <= greedy, (n, count, greedy)
        assert len(plan_tiled(n, ops, masks)) == count, n
        better += count < greedy
    assert better > 0                                                 # (the search finds something on lists this small too)
    for n in (28, 30):
        count, masks = _bench_search(n)
        assert count <= len(ti.plan(n, _bench_ops(n)))
        assert len(plan_tiled(n, _bench_ops(n), masks)) == count


def test_bench_workload_searched_pass_count():
    """The 28-qubit depth-40 bench circuit: 16 passes from the search at its default beam width with qubits 0, 1, 2 on the
    line bits -- the triple the engine's layout choice ranks first by the tile-cost model among its minimum-pass triples
    (runner/engine.choose_plan_layout) -- against 18 from the greedy builder there (test_bench_workload_pass_count) and
    17 from the best of 385 greedy plans before; 18 (greedy 20) at 30 qubits."""
    assert _bench_search(28)[0] == 16
    assert _bench_search(30)[0] == 18
    from quantum_simulations_amd.runner.engine import choose_plan_layout
    l2p, masks, info = choose_plan_layout(28, [_bench_ops(28)], n_candidates=0)
    assert info["passes_chosen"] == 16 and info["passes_identity"] == 18 and sorted(l2p[:3]) == [0, 1, 2]
    assert sum(len(m) for m in masks) == 16
    moved = [([l2p[q] for q in qs], U) for qs, U in _bench_ops(28)]
    assert len(plan_tiled(28, moved, masks[0])) == 16                 # the placed layout does not grow the plan


def test_plan_search_rejects_bad_input():
    H = orc.gate_matrix("H")
    nq, qubits, mats = pack_ops([([0], H), ([1], H)])
    count = C.c_int32()
    lib = _lib.load()
    assert lib.qsim_plan_search(4, 2, _ptr(nq), _ptr(qubits), _ptr(mats), 0, None, 0, C.byref(count)) == -1   # below the fused-pass minimum
    assert lib.qsim_plan_search(9, 2, _ptr(nq), _ptr(qubits), _ptr(mats), 0, None, 0, None) == -1
    out = np.zeros(1, dtype=np.uint64)
    ops = _random_ops(14, 150, 5)
    nq, qubits, mats = pack_ops(ops)
    assert lib.qsim_plan_search(14, len(nq), _ptr(nq), _ptr(qubits), _ptr(mats), 0, _ptr(out), 1, C.byref(count)) == -1   # too small a buffer
    assert lib.qsim_plan_search(14, len(nq), _ptr(nq), _ptr(qubits), _ptr(mats), 0, None, 0, C.byref(count)) == 0 and count.value > 1
