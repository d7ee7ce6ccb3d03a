"""The directed op lists of tests/engine_cases.py reach every branch-table entry of the fused-pass gate engine that
the planner can emit -- proven on the CPU: `qsim_plan_ops` plans each list without a device and the record streams
are read back (tests/tile_interpreter.py).  tests/test_gpu_engine_cases.py runs the same lists on the device, so
this file is what says WHICH case each of those device tests executes.  Needs the built library, no GPU."""
import os

import numpy as np
import pytest

from tests import engine_cases as ec
from tests import tile_interpreter as ti
from tests.test_gpu_kernels import _random_ops

CASES = ec.directed_lists()


@pytest.fixture(scope="module")
def planned():
    """case id -> (case, planned images)"""
    return {ec.case_id(c): (c, ti.plan(c.n, c.ops)) for c in CASES}


def test_table_and_unreachable_list():
    assert len(ec.table()) == 109
    assert sorted(set(ec.WIDTH.values())) == [1, 4, 8, 9]
    listed = [(f, v) for f, v, _, _ in ec.UNREACHABLE]
    assert len(set(listed)) == len(listed) and set(listed) <= ec.table()
    assert len(listed) <= 13 + 3
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "quantum_simulations_amd", "csrc")
    planner = ""
    for name in ("tile_ops.h", "tile_groups.h", "tile_planner.h"):     # the planner sources
        with open(os.path.join(csrc, name)) as f:
            planner += " ".join(f.read().split()) + " "
    for f, v, line, why in ec.UNREACHABLE:           # the quoted rule is a line of the planner as it stands
        assert why and " ".join(line.split()) in planner, (f, v, line)


def test_every_list_is_planned_as_aimed(planned):
    """Each list is ONE pass of the engine text it names and holds the (family, variant, predicate form) of its id."""
    for cid, (c, images) in planned.items():
        assert 2 <= len(c.ops) <= 8, cid
        assert len(images) == 1, cid
        assert int(images[0]["T"]) == min(c.n, 11), cid
        assert (c.text, c.family, c.variant, c.form) in ec.ledger_of_images(images), (cid, sorted(ec.ledger_of_images(images)))
        assert max(float(np.max(np.abs(U))) for _, U in c.ops) <= 1.0, cid


@pytest.mark.parametrize("text", [ec.FULL, ec.PARTIAL])
def test_directed_lists_cover_the_table(planned, text):
    """Coverage is an equality: the entries the lists reach == the table minus UNREACHABLE, in each engine text; every
    entry under every predicate form it can take (engine_cases.possible_forms), and under no other."""
    seen = set()
    for c, images in planned.values():
        seen |= {e[1:] for e in ec.ledger_of_images(images) if e[0] == text}
    assert {(f, v) for f, v, _ in seen} == ec.table() - {(f, v) for f, v, _, _ in ec.UNREACHABLE}
    assert seen == ec.required(text)
    # every entry runs unpredicated somewhere -- except register mask 0 of the phase families, whose bits are all in
    # the predicate (a phase gate has at least one bit)
    bare = {(f, v) for f, v, form in seen if form == "none"}
    assert ec.table() - {(f, v) for f, v, _, _ in ec.UNREACHABLE} - bare == {(f, 0) for f in ec._PHASES}
    # ... and by the list AIMED at it (the test id names it)
    aimed = {(c.family, c.variant, c.form) for c in CASES if c.text == text}
    assert aimed == ec.required(text)


def test_sizes_and_direct_layouts(planned):
    """PARTIAL: every required entry at 8, 9 and 10 qubits (the three tile sizes).  FULL: at 11 qubits (one tile)
    without the outer forms and at 14 with them; images of all four direct-in / direct-out combinations at both."""
    for n in ec.PARTIAL_SIZES:
        assert {(c.family, c.variant, c.form) for c in CASES if c.n == n} == ec.required(ec.PARTIAL), n
    at = {n: {(c.family, c.variant, c.form) for c in CASES if c.n == n} for n in ec.FULL_SIZES}
    assert at[14] == ec.required(ec.FULL)
    assert at[11] == {e for e in ec.required(ec.FULL) if "outer" not in e[2]}
    assert 11 in ec.FULL_SIZES and max(ec.FULL_SIZES) >= 13
    for n in ec.FULL_SIZES:
        flags = set()
        for c, images in planned.values():
            if c.n == n:
                flags |= ec.direct_flags(images)
        assert flags == {(False, False), (False, True), (True, False), (True, True)}, (n, flags)
    # a sunk swap of a full tile has a write-back behind it
    for c, images in planned.values():
        if c.text == ec.FULL and c.family == "ASWAP1":
            assert ec.direct_flags(images) == {(False, False)}, ec.case_id(c)


def test_planner_emits_nothing_unreachable(planned):
    """Neither on the directed lists nor on the random lists of test_fused_tile_passes_vs_oracle: every record is an
    entry outside UNREACHABLE under a predicate form possible_forms allows."""
    def check(images, what):
        for text, f, v, form in ec.ledger_of_images(images):
            assert form in ec.possible_forms(text, f, v), (what, text, f, v, form)
    for cid, (_, images) in planned.items():
        check(images, cid)
    for n in (8, 9, 10, 11, 12, 13, 16, 18):
        for seed in range(3):
            check(ti.plan(n, _random_ops(n, 90, 50 * n + seed)), (n, seed))


def test_interpreter_equals_the_longdouble_reference(planned):
    """The numpy walk of the planned records == the gate-by-gate extended-precision reference, to 1e-13, for every
    directed list: the lists, the planner's records and the reference agree before a device is involved."""
    for seed, (cid, (c, images)) in enumerate(planned.items()):
        psi = ec.random_state(c.n, 1000 + seed)
        want = ec.reference(psi, c.ops)
        ti.run(psi, images)
        assert float(np.max(np.abs(psi - want))) <= 1e-13, cid


def test_reference_conventions():
    """The reference follows the ABI: qubit q is index bit q, a 2q matrix is big-endian inside its pair."""
    psi = np.zeros(8, dtype=complex)
    psi[0b001] = 1.0                                          # qubit 0 set
    out = ec.reference(psi, [([0, 2], np.eye(4)[[0, 1, 3, 2]])])   # CNOT: control = first qubit of the pair
    assert abs(out[0b101] - 1) == 0 and abs(out).sum() == 1
    out = ec.reference(psi, [([2, 0], np.eye(4)[[0, 1, 3, 2]])])   # control qubit 2 is 0: nothing moves
    assert abs(out[0b001] - 1) == 0
    out = ec.reference(psi, [([0], np.array([[1, 2], [3, 4]]))])
    assert out[0] == 2 and out[1] == 4
    assert out.dtype == np.clongdouble
