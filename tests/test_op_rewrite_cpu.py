"""The host-side op-list rewrite (csrc/op_rewrite.h, `qsim_rewrite_ops`, `planner.rewrite_ops`) on the CPU: the rewritten
list gives the amplitudes of the caller's list, needs no more tiles, is a fixed point, and brings the bench circuits to
15 / 17 searched passes or fewer.  No device involved."""
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
from tests.test_gpu_kernels import _rand_state, _rand_unitary
from tests.test_pass_search_cpu import _bench_ops

EQUIV_TOL = 1e-13                  # rewritten list against the caller's list on a random state
REPLAY_TOL = 1e-12                 # interpreter replay of the planned rewritten list against the oracle

_NAMES_1Q = ("H", "X", "Y", "Z", "S", "T", "RY", "G", "COLLAPSE")
_NAMES_2Q = ("CNOT", "CNOT", "CNOT", "CZ", "CY", "CR", "SWAP", "U4")


def collapse_factor(kind: int, scale: float) -> np.ndarray:
    """The four 2x2 factors a measurement or reset leaves (runner/dynamic.py): |0><0|, |1><1|, |0><0|, |0><1|, scaled."""
    m = np.zeros((2, 2), dtype=np.complex128)
    m[(0, 1, 0, 0)[kind], (0, 1, 0, 1)[kind]] = scale
    return m


def _one_op(n, rng, tag, collapse):
    if rng.random() < 0.55:
        name = _NAMES_1Q[int(rng.integers(len(_NAMES_1Q)))]
        q = [int(rng.integers(n))]
        if name == "COLLAPSE":
            # rare, and close to 1 in scale: a list of 100 ops keeps a state worth comparing
            rare = rng.random() < 0.25
            return (q, collapse_factor(int(rng.integers(4)), float(rng.uniform(1.0, 1.3)))) if collapse and rare else (q, orc.gate_matrix("H"))
        return q, orc.gate_matrix(name, {"theta": float(rng.uniform(0, 2 * np.pi)), "p": int(rng.integers(2, 6))})
    name = _NAMES_2Q[int(rng.integers(len(_NAMES_2Q)))]
    qs = [int(x) for x in rng.choice(n, size=2, replace=False)]
    if name == "U4":
        return qs, _rand_unitary(4, tag)
    return qs, orc.gate_matrix(name, {"k": int(rng.integers(2, 6))})


def mixed_ops(n, n_ops, seed, framed=False, collapse=True):
    """A seeded list drawn from H, X, Y, Z, S, T, RY, G, CNOT, CZ, CY, CR, SWAP, a dense 2q and the collapse factors;
    framed: it starts and ends with X / Y on the controls of its first and last CNOTs."""
    rng = np.random.default_rng(seed)
    ops = [_one_op(n, rng, seed * 1000 + i, collapse) for i in range(n_ops)]
    if framed:
        cnot = orc.gate_matrix("CNOT")
        a, b, c, d = (int(x) for x in rng.choice(n, size=4, replace=False))
        ops = ([([a], orc.gate_matrix("X")), ([c], orc.gate_matrix("Y")), ([a, b], cnot), ([c, d], cnot)] + ops +
               [([b, a], cnot), ([d, c], cnot), ([b], orc.gate_matrix("Y")), ([d], orc.gate_matrix("X"))])
    return ops


@functools.lru_cache(maxsize=None)
def _lists():
    """(n, ops) of the seeded lists every test below walks: 6..10 qubits, 40..120 ops, every third one framed."""
    out = []
    for seed in range(30):
        n = 6 + seed % 5
        out.append((n, mixed_ops(n, 40 + (37 * seed) % 81, 7000 + seed, framed=seed % 3 == 0)))
    return out


def _same(a, b):
    return len(a) == len(b) and all(x[0] == y[0] and np.array_equal(x[1], y[1]) for x, y in zip(a, b))


def _need_tile(n, ops):
    stats = {}
    planner.rewrite_ops(n, ops, stats)
    return stats["need_tile_in"]


def test_rewritten_lists_give_the_same_state():
    worst = 0.0
    for case, (n, ops) in enumerate(_lists()):
        psi = _rand_state(n, 900 + case)
        want = psi.copy()
        orc.apply_ops(want, ops)
        orc.apply_ops(psi, planner.rewrite_ops(n, ops))
        worst = max(worst, float(np.max(np.abs(psi - want))))
        np.testing.assert_allclose(psi, want, rtol=0, atol=EQUIV_TOL, err_msg=f"case {case}")
    print(f"max |diff| over {len(_lists())} lists: {worst:.2e}")


def test_structure_of_rewritten_lists():
    """No more ops that need a tile than before; no uncontrolled anti-diagonal 1q op is left except explicit X ops at the
    front (nothing precedes them on their qubit; every other op takes a pending X in, so none is forced next to one);
    rewriting a rewritten list changes nothing."""
    X = orc.gate_matrix("X")
    for case, (n, ops) in enumerate(_lists()):
        stats = {}
        out = planner.rewrite_ops(n, ops, stats)
        assert stats["ops_in"] == len(ops) and stats["ops_out"] == len(out), case
        assert stats["need_tile_out"] <= stats["need_tile_in"], (case, stats)
        assert stats["need_tile_out"] == _need_tile(n, out), case
        seen = set()
        for qs, U in out:
            if len(qs) == 1 and U[0, 0] == 0 and U[1, 1] == 0:
                assert np.array_equal(U, X) and qs[0] not in seen, (case, qs, U)
            seen.update(qs)
        again = {}
        assert _same(planner.rewrite_ops(n, out, again), out), case
        assert again["need_tile_out"] == again["need_tile_in"] == stats["need_tile_out"], case


def test_short_lists_pass_through():
    assert planner.rewrite_ops(8, []) == []
    singles = [([3], orc.gate_matrix(g, {"theta": 0.7, "p": 3})) for g in ("H", "X", "Y", "Z", "S", "T", "RY", "G")]
    singles += [([1, 5], orc.gate_matrix(g, {"k": 3})) for g in ("CNOT", "CZ", "CY", "CR", "SWAP")]
    singles += [([5, 2], _rand_unitary(4, 5))] + [([0], collapse_factor(kind, 1.25)) for kind in range(4)]
    for op in singles:
        assert _same(planner.rewrite_ops(8, [op]), [op]), op


def test_too_small_an_output_buffer_is_an_error():
    n, ops = _lists()[0]
    nq, qubits, mats = pack_ops(ops)
    full = len(planner.rewrite_ops(n, ops))
    lib, count = _lib.load(), C.c_int32()
    room = full - 1
    out_nq, out_q, out_m = np.full(room, -7, dtype=np.int32), np.zeros(2 * room, dtype=np.int32), np.zeros((room, 16), dtype=np.complex128)
    head = (n, len(nq), _ptr(nq), _ptr(qubits), _ptr(mats))
    assert lib.qsim_rewrite_ops(*head, _ptr(out_nq), _ptr(out_q), _ptr(out_m), room, C.byref(count), None) == _lib.QSIM_ERR_INVALID
    assert count.value == full and (out_nq == -7).all()                      # the count asked for; nothing written
    assert lib.qsim_rewrite_ops(*head, None, None, None, 0, C.byref(count), None) == _lib.QSIM_ERR_INVALID
    assert lib.qsim_rewrite_ops(*head, _ptr(out_nq), _ptr(out_q), _ptr(out_m), room, None, None) == _lib.QSIM_ERR_INVALID
    bad = qubits.copy()
    bad[0] = n
    assert lib.qsim_rewrite_ops(n, len(nq), _ptr(nq), _ptr(bad), _ptr(mats), _ptr(out_nq), _ptr(out_q), _ptr(out_m), room, C.byref(count), None) != 0


@functools.lru_cache(maxsize=None)
def _bench_rewritten(n):
    stats = {}
    return planner.rewrite_ops(n, _bench_ops(n), stats), stats


@pytest.mark.parametrize("n, need_tile, passes", [(28, 363, 15), (30, 401, 17)])
def test_bench_circuits_need_fewer_tiles_and_passes(n, need_tile, passes):
    """The depth-40 bench circuits: 586 -> at most 363 ops that need a tile and 16 -> at most 15 searched passes at 28
    qubits, 654 -> at most 401 and 18 -> at most 17 at 30 (default beam, qubits 0, 1, 2 on the line bits)."""
    ops, stats = _bench_rewritten(n)
    print(n, stats)
    assert stats["need_tile_in"] == (586 if n == 28 else 654) and stats["need_tile_out"] <= need_tile
    assert stats["ops_out"] <= stats["ops_in"]
    masks = planner.search_tiles(n, ops)
    print(n, "searched passes:", len(masks))
    assert len(masks) <= passes
    assert len(planner.plan_ops(n, ops, masks)) == len(masks)


def test_layout_choice_of_the_rewritten_bench_circuit():
    from quantum_simulations_amd.runner.engine import choose_plan_layout
    ops, _ = _bench_rewritten(28)
    l2p, masks, info = choose_plan_layout(28, [ops], n_candidates=0)
    assert info["passes_chosen"] <= 15 and sorted(l2p[:3]) == [0, 1, 2], info
    assert sum(len(m) for m in masks) == info["passes_chosen"]
    moved = [([l2p[q] for q in qs], U) for qs, U in ops]
    assert planner.pass_count(28, moved, masks[0]) == info["passes_chosen"]       # the placed layout does not grow the plan


def device_cases(n):
    """(name, op list) of the circuits tests/test_gpu_op_rewrite.py runs on the device, as the engine batches them."""
    from quantum_simulations_amd import circuits as gen
    from quantum_simulations_amd.circuit.fusion import batch_levels
    from quantum_simulations_amd.circuit.io import levelize, validate_circuit_dict
    out = []
    for name, cd in (("random", gen.random_1q_cx_circuit(n, depth=20, seed=150 + n)),
                     ("clifford_t", gen.random_clifford_t_circuit(n, depth=40, seed=160 + n))):
        batches = [p["local_ops"] for p in batch_levels(levelize(validate_circuit_dict(cd)), n)]
        assert len(batches) == 1
        out.append((name, cd, batches[0]))
    out.append(("mixed", None, mixed_ops(n, 90, 170 + n, framed=True, collapse=False)))
    return out


@pytest.mark.parametrize("n", [12, 14])
def test_rewritten_lists_replay_into_the_oracle_state(n):
    """The lists the device test runs: rewritten, searched, planned under the searched tiles and executed by the
    interpreter, they give the oracle's state of the ORIGINAL list."""
    for name, _, ops in device_cases(n):
        rewritten = planner.rewrite_ops(n, ops)
        masks = planner.search_tiles(n, rewritten)
        images = planner.plan_ops(n, rewritten, masks)
        assert len(images) == len(masks), name
        psi = _rand_state(n, 500 + n)
        want = psi.copy()
        orc.apply_ops(want, ops)
        ti.run(psi, images)
        np.testing.assert_allclose(psi, want, rtol=0, atol=REPLAY_TOL, err_msg=name)
