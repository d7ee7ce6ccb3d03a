"""Staging method "tiles" on the CPU (runner/partition_plan.py + the library's pass builder in peek mode, no device):
what `qsim_plan_peek_pass` answers, and that a planned partition schedule -- executed step by step on a full state vector
with the re-layouts as qubit swaps -- is the circuit (amplitudes against the oracle), for every circuit family, 2 / 4 / 8
ranks, every thin-pass threshold."""
import numpy as np
import pytest

from oracle import dense_oracle as orc
from quantum_simulations_amd import circuits as gen
from quantum_simulations_amd.circuit.fusion import fuse_1q_ops
from quantum_simulations_amd.circuit.io import validate_circuit_dict
from quantum_simulations_amd.kernel import gates as gt, planner
from quantum_simulations_amd.kernel.device import pack_ops
from quantum_simulations_amd.runner import partition_plan as pp


def _ops(cd):
    cd = validate_circuit_dict(cd)
    return fuse_1q_ops([(g["qubits"], gt.gate_matrix(g["gate"], g["params"])) for g in cd["gates"]])


def _peek(k, n, ops, done=None, avoid=0, hint=0):
    done = np.zeros(len(ops), dtype=np.uint8) if done is None else np.asarray(done, dtype=np.uint8)
    return planner.peek_pass(k, n, *pack_ops(ops), done, np.zeros(max(1, len(ops)), dtype=np.int32), avoid, hint)


def _first_pass_of_a_full_plan(k, ops):
    images = planner.plan_ops(k, ops)
    return int(planner.tile_masks(images)[0]), len(images)


def test_peek_is_the_first_pass_of_a_full_plan_when_nothing_is_global():
    """No rank bits, nothing done: the tile the peek reports is the tile of the first pass `qsim_plan_ops` plans."""
    for n, seed in ((12, 1), (16, 2), (26, 3)):
        ops = _ops(gen.random_1q_cx_circuit(n, depth=12, seed=seed))
        mask, need, members = _peek(n, n, ops)
        first, passes = _first_pass_of_a_full_plan(n, ops)
        assert mask == first and need & ~mask == 0 and 0 < len(members) <= len(ops) and passes >= 1
        assert members == sorted(members) and bin(mask).count("1") == min(n, 11) - 3
        if n == 26:        # the fill bits of a tile are the caller's to veto (slab bits of a coming re-layout); the needed ones stay
            small = ops[:6]
            m0, need0, _ = _peek(n, n, small)
            fill = m0 & ~need0
            assert fill, "six ops cannot need all eight tile bits"
            m1, need1, _ = _peek(n, n, small, avoid=fill)
            assert need1 == need0 and m1 & fill == 0 and bin(m1).count("1") == bin(m0).count("1")


def test_peek_treats_rank_bits_as_controls_never_as_targets():
    n, k = 12, 10
    H, T, CX, CZ = gt.H(), gt.T(), gt.CNOT(), gt.CZ()
    ops = [([11], H),            # 0: targets a rank bit: waits
           ([11, 3], CX),        # 1: control on the rank bit, but behind op 0 on that qubit (H does not commute): waits
           ([10, 4], CX),        # 2: control on a rank bit, target local: runs
           ([10], T),            # 3: phase on a rank bit: runs
           ([5, 10], CZ),        # 4: diagonal with a rank bit: runs
           ([4, 10], CX),        # 5: TARGET on a rank bit: waits
           ([6], H), ([6, 7], CX)]
    mask, need, members = _peek(k, n, ops)
    assert 0 not in members and 1 not in members and 5 not in members
    assert {2, 3, 4, 6, 7} <= set(members)
    assert mask >> k == 0 and need >> k == 0                       # rank bits are never tile bits
    # what ran is not offered again; an empty pass is an answer (everything left waits for a rank bit), not an error
    done = np.ones(len(ops), dtype=np.uint8)
    done[[0, 1, 5]] = 0
    assert _peek(k, n, ops, done=done)[2] == []
    # a named tile is taken as it is (when it holds something)
    hint = (1 << 4) | (1 << 6) | (1 << 7) | (1 << 8) | (1 << 9) | (1 << 3) | (1 << 5)
    m3, _, mem3 = _peek(k, n, ops, hint=hint)
    assert m3 & hint == hint and {2, 6, 7} <= set(mem3)
    with pytest.raises(ValueError):
        _peek(k, n, [([12], H)])                                    # qubit outside the whole state
    with pytest.raises(ValueError):
        _peek(12, 10, ops)                                          # fewer total than local qubits


def _run_schedule(res, ops, n, k):
    """The steps of a partition plan on a FULL 2^n state: ops on the index bits of their time, a re-layout request ([local
    bit, rank bit], SWAP) as the swap of the two qubits; then the qubits back to where they started (`moved`)."""
    psi = np.zeros(1 << n, dtype=np.complex128)
    psi[0] = 1.0
    for st in res["steps"]:
        orc.apply_ops(psi, st["local_ops"])
        orc.apply_ops(psi, st["nonlocal_ops"])
    return orc.permute_state(psi, res["moved"])


FAMILIES = {"rand": lambda n: gen.random_1q_cx_circuit(n, depth=10, seed=3), "clifft": lambda n: gen.random_clifford_t_circuit(n, depth=14, seed=4),
            "ghz_qft": gen.generate_ghz_qft, "w_qft": gen.generate_w_qft, "qpe": lambda n: gen.generate_qpe_circuit(n - 1), "ghz": gen.generate_ghz_circuit}


@pytest.mark.parametrize("family", sorted(FAMILIES))
@pytest.mark.parametrize("n,k", [(10, 9), (11, 9), (11, 8)])
def test_a_planned_partition_schedule_is_the_circuit(family, n, k):
    cd = validate_circuit_dict(FAMILIES[family](n))
    n = cd["number_of_qubits"]
    if n <= k:
        pytest.skip("everything local")
    want = orc.simulate(cd)
    ops = _ops(cd)
    for min_ops in (1, 8, 24, 1000):
        for full_width in (True, False):
            res = pp.plan_partition(ops, n, k, min_ops=min_ops, full_width=full_width)
            # every op (but exact identities) runs exactly once; tiles are named for every pass; no rank bit in a tile
            ran = sum(len(st["local_ops"]) + sum(1 for qs, U in st["nonlocal_ops"] if not (U.shape == (4, 4) and np.array_equal(U, gt.SWAP())
                                                                                             and (qs[0] < k) != (qs[1] < k)))
                      for st in res["steps"])
            identities = sum(1 for _, U in ops if np.array_equal(U, np.eye(U.shape[0])))
            assert ran == len(ops) - identities, (ran, len(ops), identities)
            assert sum(s["passes"] for s in res["segments"]) == res["passes"] and all(m >> k == 0 for s in res["segments"] for m in s["tile_masks"])
            for st in res["steps"]:
                for qs, U in st["nonlocal_ops"]:               # what is left on rank bits: re-layout requests, controls, phases
                    if U.shape == (4, 4) and np.array_equal(U, gt.SWAP()) and (qs[0] < k) != (qs[1] < k):
                        assert min(qs) >= pp.LINE_BITS          # (a slab bit is never inside a 128-byte line)
                    else:
                        assert all(q < k for q in pp.op_targets(qs, U)), (qs, "a target on a rank bit")
            np.testing.assert_allclose(_run_schedule(res, ops, n, k), want, rtol=0, atol=1e-12, err_msg=f"{family} min_ops={min_ops} full_width={full_width}")
    best = pp.plan_partition_best(ops, n, k, threads=2)
    assert best["cost"] == min(t["cost"] for t in best["tried"]) and len(best["tried"]) == len(pp.MIN_OPS_CHOICES)
    np.testing.assert_allclose(_run_schedule(best, ops, n, k), want, rtol=0, atol=1e-12)


def test_slot_placement_keeps_the_schedule_and_moves_only_local_bits():
    """`place_slots` permutes the local index bits above the line of a whole chain of executions: the same circuit, no line
    or rank bit moved, the tiles re-filled, slab bits still outside the last tile of their segment."""
    n, k = 12, 9
    cd = validate_circuit_dict(gen.random_1q_cx_circuit(n, depth=12, seed=5))
    ops = _ops(cd)
    want = orc.simulate(cd)
    res = pp.plan_partition(ops, n, k, min_ops=8)
    executions = [res["steps"]]
    sigma, before, after = pp.place_slots(executions, k)
    assert sorted(sigma.values()) == sorted(sigma.keys()) and all(sigma[b] == b for b in range(pp.LINE_BITS)) and max(sigma) < k
    assert after <= before * 1.05
    start = [sigma.get(b, b) for b in range(n)]                       # where qubit b starts now
    moved = [sigma.get(b, b) for b in res["moved"]]
    psi = np.zeros(1 << n, dtype=np.complex128)
    psi[0] = 1.0
    for st in executions[0]:
        orc.apply_ops(psi, st["local_ops"])
        orc.apply_ops(psi, st["nonlocal_ops"])
    # the plan was written for qubits starting at bit b; after the placement qubit b starts at sigma[b] and ends at moved[b]
    got = orc.permute_state(psi, moved)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
    assert start != list(range(n)) or before == after
    for st in executions[0]:
        if "tile_masks" in st:
            assert all(bin(m).count("1") == bin(st["tile_masks"][0]).count("1") and m >> k == 0 and m & 0b111 == 0 for m in st["tile_masks"])
            assert all(nd & ~m == 0 for m, nd in zip(st["tile_masks"], st["tile_needs"]))
