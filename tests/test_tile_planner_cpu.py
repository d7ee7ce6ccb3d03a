"""The host planner of the fused passes on the CPU: `qsim_plan_ops` plans an op list without a
device, tests/tile_interpreter.py executes the emitted pass images on a numpy state following the
opcode table, and the result must equal the dense oracle.  Covers pass building, register
groups, opcode / mask encoding, merged phase runs (OPC_DIAGR) and their ordering, argument budgets."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import dense_oracle as orc
from tests import tile_interpreter as ti
from tests.test_gpu_kernels import _rand_state, _random_ops

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_PROBE_LIB = os.path.join(_ROOT, "quantum_simulations_amd", "libqsim_hip_probes.so")


def _probe_env(**knobs) -> dict:
    """Planning knobs exist in the probe build only (csrc/gate_plan.h: the product library reads nothing from the
    environment): child processes that plan under a knob load libqsim_hip_probes.so through QSIM_LIBRARY."""
    if not os.path.exists(_PROBE_LIB):
        subprocess.run(["make", "-C", os.path.join(_ROOT, "quantum_simulations_amd", "csrc"), "probes"], check=True, capture_output=True)
    return dict(os.environ, QSIM_LIBRARY=_PROBE_LIB, PYTHONPATH=_ROOT, **knobs)



@pytest.mark.parametrize("n", [8, 9, 11, 12, 14])
def test_planned_passes_equal_oracle_random_ops(n):
    for seed in range(4):
        ops = _random_ops(n, 120, 70 * n + seed)
        psi = _rand_state(n, 300 + seed)
        want = psi.copy()
        orc.apply_ops(want, ops)
        images = ti.plan(n, ops)
        assert 1 <= len(images) <= len(ops)
        ti.run(psi, images)
        np.testing.assert_allclose(psi, want, rtol=0, atol=1e-12, err_msg=f"n={n} seed={seed}")


def test_direct_layouts_of_full_tiles():
    """A full tile whose first / last register group lies above the line bits is loaded / stored in that group's
    layout (TileArgs::lay_in / lay_out, OPC_GROUP_DIRECT / OPC_END_DIRECT); the record walker checks the layouts
    against the groups, run_pass that no sunk swap is left without a write-back.  Smaller tiles never are."""
    seen_in = seen_out = total = 0
    for seed in range(6):
        for n in (11, 13, 14):
            for img in ti.plan(n, _random_ops(n, 150, 4000 + 10 * n + seed)):
                list(ti.records(img))
                seen_in += bool(int(img["order"]) & ti.DIRECT_IN)
                seen_out += bool(int(img["order"]) & ti.DIRECT_OUT)
                total += 1
    assert seen_in > total // 2 and seen_out > total // 4, (seen_in, seen_out, total)
    for img in ti.plan(9, _random_ops(9, 100, 77)):
        assert int(img["T"]) < 11 and not int(img["order"]) & (ti.DIRECT_IN | ti.DIRECT_OUT)


def test_staging_swap_lists_on_line_bits_plan():
    """The chunked runner applies a staging SWAP list whose local bits lie inside a 128-B line as ONE fused pass of
    SWAP gates (runner/single_node.py): every such list must plan (regression: the first group's preference for a
    triple above the line bits once picked a triple that held no op) and act as the permutation."""
    import itertools
    SW = orc.gate_matrix("SWAP", {})
    for n in (9, 11, 12):
        for m in (1, 2, 3):
            for los in itertools.combinations(range(4), m):
                ops = [([lo, hi], SW) for lo, hi in zip(los, range(n - m, n))]
                images = ti.plan(n, ops)
                if los == (0, 1, 2) or m == 1:
                    psi = _rand_state(n, 7 * n + m)
                    want = psi.copy()
                    orc.apply_ops(want, ops)
                    ti.run(psi, images)
                    np.testing.assert_allclose(psi, want, rtol=0, atol=1e-13)


def test_two_qubit_heavy_lists_plan_and_run():
    """Lists made of dense 4x4 gates only (each claims two register bits, so groups hold one or two of them): random
    pairs, many seeds, full and partial tiles -- every list plans, and the planned passes equal the oracle."""
    rng = np.random.default_rng(4242)
    for case in range(40):
        n = int(rng.integers(8, 14))
        ops = []
        for _ in range(int(rng.integers(1, 12))):
            a, b = (int(x) for x in rng.choice(n, size=2, replace=False))
            g = rng.standard_normal((4, 4)) + 1j * rng.standard_normal((4, 4))
            q, _ = np.linalg.qr(g)
            ops.append(([a, b], q if rng.random() < 0.5 else orc.gate_matrix("SWAP", {})))
        psi = _rand_state(n, 600 + case)
        want = psi.copy()
        orc.apply_ops(want, ops)
        ti.run(psi, ti.plan(n, ops))
        np.testing.assert_allclose(psi, want, rtol=0, atol=1e-12, err_msg=str(case))


def test_outer_controlled_gate_merges_with_the_1q_gate_on_its_target():
    """A controlled gate whose control lies outside the tile, next to a plain 1q gate U on its target, is written as
    two predicated 2x2 records (control = 1: U V or V U; control = 0: U under OPC_PRED_OUTER_ZERO) instead of V + U
    (csrc/tile_groups.h, GroupEmitter::mux_pairs).  Both orders, CNOT and CY, a gate in between on another qubit, and
    the cases that must NOT pair (a gate on the target in between; a control inside the tile)."""
    n = 13
    H, X, RY, T, Y = (orc.gate_matrix(g, {"theta": 0.7}) for g in ("H", "X", "RY", "T", "Y"))
    CNOT, CY = orc.gate_matrix("CNOT", {}), orc.gate_matrix("CY", {})
    fill = [([q], H) for q in (3, 4, 7, 8, 9, 10)]  # with targets 5 and 6 the tile's high bits are 3..10: qubits 11, 12 stay outside

    def zero_records(ops):
        return sum(1 for img in ti.plan(n, ops) for r in ti.records(img) if r[0] == "gate" and r[3] < 0)

    cases = [
        (fill + [([12, 5], CNOT), ([5], RY)], 1),                       # V then U
        (fill + [([5], RY), ([12, 5], CNOT), ([5], T)], 1),             # U then V (something later touches the target)
        (fill + [([12, 5], CY), ([7], RY), ([5], RY)], 1),              # a gate on another qubit in between
        (fill + [([12, 5], CNOT), ([12, 6], CNOT), ([5], RY), ([6], Y)], 2),
        (fill + [([12, 5], CNOT), ([5], T), ([5], RY)], 0),             # T on the target sits in between
        (fill + [([4, 5], CNOT), ([5], RY)], 0),                        # control inside the tile
        (fill + [([5], RY), ([12, 5], CNOT)], 0),                       # nothing later on the target: the CNOT sinks instead
    ]
    for seed, (ops, want_zero) in enumerate(cases):
        psi = _rand_state(n, 70 + seed)
        want = psi.copy()
        orc.apply_ops(want, ops)
        ti.run(psi, ti.plan(n, ops))
        np.testing.assert_allclose(psi, want, rtol=0, atol=1e-13, err_msg=str(seed))
        assert zero_records(ops) == want_zero, (seed, zero_records(ops))


def test_phase_runs_are_merged_and_ordered():
    """QFT: the CR(k, a), CR(k, b), CR(k, c) of a register group share one descriptor, and every
    merged run is written out before the next Hadamard on one of its bits."""
    from quantum_simulations_amd.circuit.io import validate_circuit_dict
    from quantum_simulations_amd.circuits import generate_ghz_qft
    from quantum_simulations_amd.runner.engine import gate_ops
    n = 13
    cd = validate_circuit_dict(generate_ghz_qft(n))
    ops = gate_ops(cd)
    images = ti.plan(n, ops)
    psi = np.zeros(1 << n, dtype=np.complex128)
    psi[0] = 1
    descriptors = ti.run(psi, images)
    np.testing.assert_allclose(psi, orc.simulate(cd), rtol=0, atol=1e-12)
    assert descriptors < len(ops)                                   # merging happened
    assert any(rec[0] == "gate" and ti.OPC["DIAGR"] <= rec[1] < ti.OPC["DIAGR"] + 4
               for img in images for rec in ti.records(img))


def test_commuting_1q_gates_are_fused():
    """Library-side fusion of 1q gates across ops they commute with (csrc/tile_ops.h commute_fuse_1q): X through
    CNOT targets, Z / S / T through controls and CZ / CR; H must NOT pass a CNOT.  Fewer records, same state."""
    if os.environ.get("QSIM_TILE_COMMUTE_FUSE") != "2":
        # off by default (measured neutral); the knob is read once per process: run this test alone in a child
        out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", __file__ + "::test_commuting_1q_gates_are_fused"],
                             cwd=_ROOT, env=_probe_env(QSIM_TILE_COMMUTE_FUSE="2"), capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
        return
    H, X, Z, S, T = (orc.gate_matrix(g, {}) for g in ("H", "X", "Z", "S", "T"))
    CNOT, CZ = orc.gate_matrix("CNOT", {}), orc.gate_matrix("CZ", {})
    n = 9
    for seed in range(3):                         # random circuits under the fusion: same state as the oracle
        ops = _random_ops(12, 150, 8800 + seed)
        psi = _rand_state(12, 8900 + seed)
        want = psi.copy()
        orc.apply_ops(want, ops)
        ti.run(psi, ti.plan(12, ops))
        np.testing.assert_allclose(psi, want, rtol=0, atol=1e-12, err_msg=str(seed))

    def records_of(ops):
        return sum(1 for img in ti.plan(n, ops) for r in ti.records(img) if r[0] == "gate")

    # (the later gate moves back to the earlier one: that order keeps the pass count of the bench circuit at 18)
    cases = [
        ([([4], H), ([1, 4], CNOT), ([4], X)], [([4], X @ H), ([1, 4], CNOT)]),        # X passes the target
        ([([1], S), ([1, 4], CNOT), ([1], T)], [([1], T @ S), ([1, 4], CNOT)]),        # T passes the control
        ([([1], Z), ([1, 4], CZ), ([4, 1], CZ), ([1], T)], [([1], T @ Z), ([1, 4], CZ), ([4, 1], CZ)]),
        ([([4], X), ([1, 4], CNOT), ([4], X)], [([1, 4], CNOT)]),                      # X X = 1 across the target
        ([([4], H), ([1, 4], CNOT), ([4], H)], None),          # H does not commute with the CNOT on its target
        ([([1], X), ([1, 4], CNOT), ([1], X)], None),          # X on the CONTROL does not commute either
        ([([4], X), ([1, 4], CNOT), ([4], H)], None),          # H (the gate that would move) cannot pass the CNOT
    ]
    for seed, (ops, fused_by_hand) in enumerate(cases):
        psi = _rand_state(n, 50 + seed)
        want = psi.copy()
        orc.apply_ops(want, ops)
        ti.run(psi, ti.plan(n, ops))
        np.testing.assert_allclose(psi, want, rtol=0, atol=1e-13, err_msg=str(seed))
        if fused_by_hand is not None:
            assert records_of(ops) == records_of(fused_by_hand) < len(ops), seed
        else:
            assert records_of(ops) >= len(ops), seed          # nothing merged (a Hadamard scale record may be added)


def test_bench_workload_pass_count():
    """The 28-qubit depth-40 bench circuit plans into 18 passes with the two-deep tile-bit look-ahead
    (19 one deep, 24 with the first-come rule alone); planning needs no device."""
    from quantum_simulations_amd.circuit.fusion import batch_levels
    from quantum_simulations_amd.circuit.io import levelize, validate_circuit_dict
    from quantum_simulations_amd.circuits import random_1q_cx_circuit
    cd = validate_circuit_dict(random_1q_cx_circuit(28, depth=40))
    total = sum(len(ti.plan(28, p["local_ops"])) for p in batch_levels(levelize(cd), 28))
    if os.environ.get("QSIM_TILE_COMMUTE_FUSE", "0") != "0":
        pytest.skip("pass counts are pinned for the default planner")
    assert total == {"0": 24, "1": 19}.get(os.environ.get("QSIM_PLAN_LOOKAHEAD"), 18)


def test_argument_budget_is_respected():
    """Many dense 2q gates (272-byte records): passes are cut by the record budget of the 4 KiB argument
    block and every image stays inside it (ti.records asserts the bounds of every 64-byte fetch)."""
    n = 10
    rng = np.random.default_rng(8)
    ops = []
    for i in range(60):
        qa, qb = (int(x) for x in rng.choice(n, size=2, replace=False))
        z = rng.standard_normal((4, 4)) + 1j * rng.standard_normal((4, 4))
        ops.append(([qa, qb], np.linalg.qr(z)[0]))
    images = ti.plan(n, ops)
    assert len(images) >= 60 * 272 // (ti.IMAGE_BYTES - ti.STREAM_OFF)
    psi = _rand_state(n, 5)
    want = psi.copy()
    orc.apply_ops(want, ops)
    ti.run(psi, images)
    np.testing.assert_allclose(psi, want, rtol=0, atol=1e-12)
    for img in images:
        assert 2 < int(img["nrec"]) and sum(1 for _ in ti.records(img)) == int(img["nrec"]) - 1


def test_plan_ops_rejects_bad_input():
    H = orc.gate_matrix("H")
    with pytest.raises(NotImplementedError, match="non-local"):
        ti.plan(9, [([9], H)])
    with pytest.raises(ValueError):
        ti.plan(4, [([0], H)])                 # below the fused-pass minimum


def test_lookahead_planner_on_small_states():
    """The look-ahead is on by default only for states of >= 24 qubits; the knob is read once per
    process, so this module is re-run in ONE child process with it forced on (and once forced off)
    to execute the planned passes of the small cases above under both rules."""
    if os.environ.get("QSIM_PLANNER_CHILD"):
        pytest.skip("already inside the child run")
    for setting in ("2", "1", "0"):
        out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", __file__],
                             cwd=_ROOT, env=_probe_env(QSIM_PLAN_LOOKAHEAD=setting, QSIM_PLANNER_CHILD="1"), capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, f"QSIM_PLAN_LOOKAHEAD={setting}\n" + out.stdout[-3000:] + out.stderr[-2000:]


@pytest.mark.parametrize("n", [9, 12, 14])
def test_merged_descriptors_keep_list_order(n):
    """Merged phase runs (OPC_DIAGR) are written out late; a gate on one of their bits must still see
    them in list order.  Circuits dense in
    predicated phases (CR with few distinct controls), 1q phases and non-diagonal 1q gates on the
    same few qubits, many seeds, against the oracle."""
    for seed in range(12):
        rng = np.random.default_rng(9000 + 31 * n + seed)
        ctrls = [int(q) for q in rng.choice(n, size=3, replace=False)]
        hot = [int(q) for q in rng.choice(n, size=4, replace=False)]
        ops = []
        for _ in range(200):
            r = rng.random()
            q = hot[int(rng.integers(4))] if rng.random() < 0.7 else int(rng.integers(n))
            if r < 0.35:
                c = ctrls[int(rng.integers(3))]
                if c != q:
                    ops.append(([c, q] if rng.random() < 0.5 else [q, c], orc.gate_matrix("CR", {"k": int(rng.integers(1, 7))})))
            elif r < 0.60:
                ops.append(([q], orc.gate_matrix(("T", "R", "S", "Z")[int(rng.integers(4))], {"k": int(rng.integers(1, 7))})))
            elif r < 0.90:
                ops.append(([q], orc.gate_matrix(("H", "RY", "X", "Y")[int(rng.integers(4))], {"theta": float(rng.uniform(0, 6))})))
            else:
                t = int(rng.integers(n))
                if t != q:
                    ops.append(([q, t], orc.gate_matrix("CNOT")))
        psi = _rand_state(n, 40 + seed)
        want = psi.copy()
        orc.apply_ops(want, ops)
        images = ti.plan(n, ops)
        descriptors = ti.run(psi, images)
        np.testing.assert_allclose(psi, want, rtol=0, atol=1e-12, err_msg=f"n={n} seed={seed}")
        assert descriptors < len(ops)


def _knob_child() -> None:
    """Runs in a child process under ONE knob setting (probe library): random op lists of every kind and a layered
    1q+CX circuit are planned, the pass images interpreted, the result compared with the oracle."""
    from quantum_simulations_amd.circuit.io import validate_circuit_dict
    from quantum_simulations_amd.circuits import random_1q_cx_circuit
    from quantum_simulations_amd.runner.engine import gate_ops
    for n, n_ops, seed in ((9, 120, 1), (12, 150, 2), (14, 150, 3)):
        ops = _random_ops(n, n_ops, 6100 + seed)
        psi = _rand_state(n, 6200 + seed)
        want = psi.copy()
        orc.apply_ops(want, ops)
        ti.run(psi, ti.plan(n, ops))
        np.testing.assert_allclose(psi, want, rtol=0, atol=1e-12, err_msg=f"n={n}")
    cd = validate_circuit_dict(random_1q_cx_circuit(15, depth=14, seed=5))
    psi = np.zeros(1 << 15, dtype=np.complex128)
    psi[0] = 1
    ti.run(psi, ti.plan(15, gate_ops(cd)))
    np.testing.assert_allclose(psi, orc.simulate(cd), rtol=0, atol=1e-12)
    print("KNOB-CHILD-OK")


_KNOBS = [("QSIM_PASS_GATES", v) for v in ("1", "7", "40")] + [("QSIM_PLAN_LOOKAHEAD", v) for v in ("0", "1", "2")] + \
         [(k, "0") for k in ("QSIM_TILE_SPECIAL", "QSIM_TILE_MERGE_DIAG", "QSIM_TILE_HAD", "QSIM_TILE_GROUP_SEARCH",
                             "QSIM_TILE_SINK_SWAPS", "QSIM_TILE_DIRECT", "QSIM_TILE_MUX", "QSIM_TILE_LAST_SEARCH",
                             "QSIM_PLAN_CONFLICT_COST", "QSIM_PLAN_COMMUTE")] + \
         [("QSIM_PLAN_CONFLICT_COST", "3"), ("QSIM_PLAN_COMMUTE", "1"), ("QSIM_TILE_COMMUTE_FUSE", "1"), ("QSIM_TILE_COMMUTE_FUSE", "2"),
          ("QSIM_TILE_COMMUTE_FUSE", "3"), ("QSIM_TILE_COMMUTE_FUSE", "4"), ("QSIM_TILE_LAST_SEARCH", "3"),
          ("QSIM_PLAN_SCAN_WINDOW", "1"), ("QSIM_PLAN_SCAN_WINDOW", "24"), ("QSIM_PLAN_ANCHOR", "3"), ("QSIM_PLAN_ANCHOR", "6")]


@pytest.mark.parametrize("knob,value", _KNOBS)
def test_every_planning_knob_setting_yields_a_correct_program(knob, value):
    """csrc/gate_plan.h: 'every setting yields a correct program' -- here for every value the planner code
    distinguishes (the knobs exist in the probe build only: VERDICT r02 item 8)."""
    out = subprocess.run([sys.executable, "-c", "import tests.test_tile_planner_cpu as t; t._knob_child()"], cwd=_ROOT,
                         env=_probe_env(**{knob: value}), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "KNOB-CHILD-OK" in out.stdout, f"{knob}={value}\n" + out.stdout[-2000:] + out.stderr[-3000:]


def test_product_library_reads_no_planning_knobs():
    """The shipped library plans the bench circuit into 18 passes whatever QSIM_* says (the same knobs move the
    probe build to 24: test_bench_workload_pass_count under QSIM_PLAN_LOOKAHEAD=0)."""
    code = ("import tests.test_tile_planner_cpu as t\n"
            "from quantum_simulations_amd.circuit.fusion import batch_levels\n"
            "from quantum_simulations_amd.circuit.io import levelize, validate_circuit_dict\n"
            "from quantum_simulations_amd.circuits import random_1q_cx_circuit\n"
            "cd = validate_circuit_dict(random_1q_cx_circuit(28, depth=40))\n"
            "print('PASSES', sum(len(t.ti.plan(28, p['local_ops'])) for p in batch_levels(levelize(cd), 28)))\n")
    env = dict(os.environ, PYTHONPATH=_ROOT, QSIM_PLAN_LOOKAHEAD="0", QSIM_TILE_DIRECT="0", QSIM_PASS_GATES="5",
               QSIM_TILE_COMMUTE_FUSE="2")
    env.pop("QSIM_LIBRARY", None)
    out = subprocess.run([sys.executable, "-c", code], cwd=_ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "PASSES 18" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


@pytest.mark.parametrize("n", [12, 14, 15])
def test_commuting_ops_overtake_waiting_ones_correctly(n):
    """Round 3's pass builder lets an op run a pass EARLIER than an op in front of it that has to wait, when the two are
    diagonal (or both 1 / X) on every qubit they share.  Circuits made of exactly such neighbours -- fans of CNOTs from
    one control, fans into one target, X on targets, Z / S / T / CZ / CR on controls, with a few Hadamards and dense
    gates to end the runs -- on more qubits than a tile holds, so passes are cut in the middle of the runs."""
    CNOT, CZ, H = orc.gate_matrix("CNOT"), orc.gate_matrix("CZ"), orc.gate_matrix("H")
    for seed in range(8):
        rng = np.random.default_rng(31000 + 97 * n + seed)
        ops = []
        for _ in range(60):
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
                    ops.append(([q, hub], orc.gate_matrix("CY")))                  # Y on the target: NOT X-type
                r = rng.random()
                if r < 0.25:
                    ops.append(([hub], orc.gate_matrix("X" if kind >= 0.35 and kind < 0.7 else "T")))
                elif r < 0.35:
                    ops.append(([q], orc.gate_matrix(("Z", "S", "X", "Y")[int(rng.integers(4))])))
                elif r < 0.42:
                    ops.append(([hub if rng.random() < 0.5 else q], H))
                elif r < 0.45:
                    a, b = (int(x) for x in rng.choice(n, size=2, replace=False))
                    ops.append(([a, b], np.linalg.qr(rng.standard_normal((4, 4)) + 1j * rng.standard_normal((4, 4)))[0]))
        psi = _rand_state(n, 40 + seed)
        want = psi.copy()
        orc.apply_ops(want, ops)
        images = ti.plan(n, ops)
        assert len(images) >= 2
        ti.run(psi, images)
        np.testing.assert_allclose(psi, want, rtol=0, atol=1e-12, err_msg=f"n={n} seed={seed}")


def _long_list_with_a_control_only_qubit(n: int, n_ops: int, seed: int) -> list:
    """Qubit 0 is only ever a CNOT control: the pass builder's "every qubit is blocked" early exit never fires."""
    rng = np.random.default_rng(seed)
    H, T, CX = orc.gate_matrix("H"), orc.gate_matrix("T"), orc.gate_matrix("CNOT")
    ops = []
    for _ in range(n_ops):
        r = rng.random()
        if r < 0.5:
            ops.append(([int(rng.integers(1, n))], H if rng.random() < 0.5 else T))
        elif r < 0.6:
            ops.append(([0, int(rng.integers(1, n))], CX))
        else:
            a, b = (int(x) for x in rng.choice(np.arange(1, n), size=2, replace=False))
            ops.append(([a, b], CX))
    return ops


def test_planning_time_per_pass_is_bounded_on_long_lists():
    """with a control-only qubit every scan of the commutation-aware pass builder walked the whole remaining
    list -- 7.5-12 ms of host time per pass on a 4000-op list, several times the device time of a 28-qubit pass (1.7 ms).
    The scans now stop `plan_scan_window` waiting ops behind the front (csrc/tile_planner.h).  Budget: 6 ms per pass
    (measured 1.4-1.6 ms on the idle build container, up to 4 under a parallel test run; the unbounded scan took 7.5-12)
    -- and no more passes than the unbounded scan needed (100)."""
    import time

    from quantum_simulations_amd.kernel import planner
    from quantum_simulations_amd.kernel.device import pack_ops
    if os.environ.get("QSIM_PLANNER_CHILD"):
        pytest.skip("pass count and budget are those of the default planner, not of a forced look-ahead setting")
    n = 28
    packed = pack_ops(_long_list_with_a_control_only_qubit(n, 4000, 1))
    best = 1e9
    for _ in range(3):
        t0 = time.perf_counter()
        k = planner.pass_count(n, packed)
        best = min(best, time.perf_counter() - t0)
    assert k <= 102, k
    assert best / k < 6e-3, f"{best / k * 1e3:.2f} ms of planning per pass"


def test_bounded_scan_plans_equal_the_oracle_on_lists_longer_than_the_window():
    """Op lists of several scan windows (default 384 waiting ops) on 13 qubits, control-only qubit included: planned,
    interpreted, compared with the oracle."""
    n = 13
    for seed in (5, 6):
        ops = _long_list_with_a_control_only_qubit(n, 2500, seed)
        psi = _rand_state(n, 900 + seed)
        want = psi.copy()
        orc.apply_ops(want, ops)
        ti.run(psi, ti.plan(n, ops))
        np.testing.assert_allclose(psi, want, rtol=0, atol=1e-11)
