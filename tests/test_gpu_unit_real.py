"""Unit-diagonal butterflies for real 2x2 gates (OPC_UNIT1) on the device: every one of the engine's twelve cases (target
register 0..2 x form D / A x sigma = +-1), in register groups made of the line bits, in the group a full tile is loaded in,
the one it is stored from and one between them, in partial tiles (9 qubits) and in tiles with index bits outside them
(12, 13 qubits), 1, 2 and 12 such records in a pass, mixed with H, with a complex 2x2 in the pass to take the
factors and without one.  tests/test_unit_real_cpu.py shows on the CPU which records the lowering rewrites; here
`planner.lower_images` of the same plan names the cases each list reaches, the device state is set against
oracle/dense_oracle.py at the fused-engine tests' bound (1e-12 absolute) from a random state, and the norm stays within
1e-13; the group lists once more with the lowering switched off (a child process on the probe build,
QSIM_TILE_UNIT=0): agreement within 1e-14.  Seen on an MI355X over all lists: |device - oracle| <= 7.1e-17,
|norm2 after - norm2 before| <= 2.5e-15, |on - off| <= 6.0e-17."""
import numpy as np
import pytest

from oracle import dense_oracle as orc
from quantum_simulations_amd.kernel import planner
from tests.test_gpu_kernels import ATOL_KERNEL, _rand_state, _rand_unitary
from tests.test_unit_real_cpu import ANGLES, UNIT1, H, X, Z, cases_of, family, qualifies, ry, unit_records

pytestmark = pytest.mark.gpu

NORM_TOL = 1e-13
SIZES = (11, 9, 12, 13)


@pytest.fixture(scope="module")
def chunks():
    from quantum_simulations_amd.kernel.device import DeviceChunk, device_count
    assert device_count() >= 1
    held = {n: DeviceChunk.empty(n) for n in SIZES}
    worst = {}
    yield held, worst
    for key, w in sorted(worst.items()):
        print(f"\nunit-real max {key}: {w:.3e}", end="")
    print()
    for dev in held.values():
        dev.close()


def _run(held, worst, n, ops, seed, want_units=None):
    """ops on a random state of n qubits: device against oracle; returns the OPC_UNIT1 variants of the lowered plan"""
    images = planner.plan_ops(n, ops)
    low, count = planner.lower_images(images)
    variants = {c - UNIT1 for c in cases_of(low) if UNIT1 <= c < UNIT1 + 12}
    if want_units is not None:
        assert count == want_units, (count, want_units)
    psi0 = _rand_state(n, seed)
    want = psi0.copy()
    orc.apply_ops(want, ops)
    dev = held[n]
    dev.upload(psi0)
    before = dev.norm2()
    passes = dev.apply_ops(ops, fused=True)
    after = dev.norm2()
    got = dev.download()
    assert passes == len(images)
    err = float(np.max(np.abs(got - want)))
    worst["|device - oracle|"] = max(worst.get("|device - oracle|", 0.0), err)
    worst["|norm2 after - before|"] = max(worst.get("|norm2 after - before|", 0.0), abs(after - before))
    print(f"n {n}: {len(ops)} ops, {count} OPC_UNIT1 records {sorted(variants)}, max |device - oracle| {err:.3e}, norm2 {before:.15f} -> {after:.15f}")
    assert err <= ATOL_KERNEL
    assert abs(after - before) <= NORM_TOL
    return variants


def _triples(n):
    """register groups of a pass on n qubits (tile = index bits 0..min(n, 11) - 1): the line bits; for a full tile the
    groups above them"""
    T = min(n, 11)
    return [(0, 1, 2)] + ([(T - 3, T - 2, T - 1)] if T < 11 else [(5, 6, 7), (8, 9, 10)])


def _four_kinds(theta_d, theta_a):
    """(form D, +), (form D, -), (form A, +), (form A, -): RY at a small and at a large half angle, and each times Z"""
    return [ry(theta_d), ry(theta_d) @ Z, ry(theta_a), ry(theta_a) @ Z]


def group_lists(n, host, k):
    kinds = _four_kinds(0.9, 2.4)
    ops = []
    for t, triple in enumerate(_triples(n)):
        for j, q in enumerate(triple):
            ops.append(([q], kinds[(k + j + t) % 4]))
            ops.append(([q], H if (j + t) % 2 else kinds[(k + j + t + 1) % 4] @ X))
    if n > 11:                     # a tile with outer bits: gates on them make a second pass
        ops += [([n - 1], kinds[k]), ([n - 2], H)]
    if host == "complex":
        ops.insert(3, ([3], _rand_unitary(2, 77 + k)))
    return ops


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("host", ["complex", "none"])
def test_every_case_in_every_group(chunks, n, host):
    """Each of the four kinds on each register of each group, three groups in one pass for a full tile; with a complex
    2x2 in the pass and without (the last record of the family then stays OPC_REAL1 and carries the factors)."""
    held, worst = chunks
    seen = set()
    for k in range(4):
        seen |= _run(held, worst, n, group_lists(n, host, k), 4000 + 10 * n + k)
    # the four lists reached all twelve cases (target register x form x sign) on the device
    assert seen == set(range(12)), sorted(seen)


@pytest.mark.parametrize("n", [11, 9])
def test_the_angle_list(chunks, n):
    """RY, RY X, X RY, RY Z, Z RY at 0, 1e-9, pi/2 -+ 1e-9, pi/2 (the tie of the two forms), pi, 3 pi/2, 2 pi - 1e-9 and
    20 seeded angles: twelve records of the family per pass, on every register of two groups."""
    held, worst = chunks
    T = min(n, 11)
    qubits = [0, 1, 2, T - 3, T - 2, T - 1]
    mats = [M for theta in ANGLES for M in family(theta).values()]
    lowered = 0
    for i in range(0, len(mats), 12):
        ops = [([qubits[j % 6]], M) for j, M in enumerate(mats[i:i + 12])]
        ops.insert(5, ([3], _rand_unitary(2, 300 + i)))
        # (the complex 2x2 takes the factors: every gate of the family in the list is lowered, none of the others)
        count = sum(qualifies(M) for M in mats[i:i + 12])
        _run(held, worst, n, ops, 5000 + n + i, want_units=count)
        lowered += count
    assert lowered >= 100


@pytest.mark.parametrize("count", [1, 2, 12])
@pytest.mark.parametrize("host", ["complex", "none"])
def test_one_two_and_twelve_records_in_a_pass(chunks, count, host):
    held, worst = chunks
    n = 11
    rng = np.random.default_rng(count)
    qubits = [0, 1, 2, 5, 6, 7, 8, 9, 10, 3, 4, 5]
    ops = []
    for i in range(count):
        ops.append(([qubits[i]], ry(float(rng.uniform(0, 2 * np.pi))) @ (Z if i % 3 == 1 else np.eye(2))))
        if i % 2 == 0:
            ops.append(([qubits[(i + 1) % 12]], H))
    if host == "complex":
        ops.append(([4], _rand_unitary(2, 900 + count)))
    # without a complex 2x2 one record of the family stays OPC_REAL1 to carry the factors (a single one is left alone)
    _run(held, worst, n, ops, 6000 + count, want_units=count if host == "complex" else max(count - 1, 0))


def group_states():
    """name -> device state of every list of test_every_case_in_every_group, from that test's random states, under
    whatever library and switches the process runs with"""
    from quantum_simulations_amd.kernel.device import DeviceChunk
    states = {}
    for n in SIZES:
        dev = DeviceChunk.empty(n)
        for host in ("complex", "none"):
            for k in range(4):
                dev.upload(_rand_state(n, 4000 + 10 * n + k))
                dev.apply_ops(group_lists(n, host, k), fused=True)
                states[f"{n}_{host}_{k}"] = dev.download()
        dev.close()
    return states


def test_lowering_on_against_off(tmp_path):
    """The 32 group lists with the lowering on (this process, the product library) against off: a fresh child process
    that loads the probe build with QSIM_TILE_UNIT=0 -- the product library reads no switch -- and leaves its states in a
    file.  OPC_UNIT1 and OPC_REAL1 differ in a few roundings per gate on normalised states: agreement within 1e-14."""
    import os
    import subprocess
    import sys
    from quantum_simulations_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    probe = os.path.join(root, "quantum_simulations_amd", "libqsim_hip_probes.so")
    assert os.path.exists(probe), "the probe build is made by build() / `make probes`"
    assert os.path.basename(str(_lib.LIB_PATH)) == _lib.LIB_NAME, "this process must run the product library"
    out = str(tmp_path / "states_off.npz")
    env = dict(os.environ, QSIM_LIBRARY=probe, QSIM_TILE_UNIT="0")
    subprocess.run([sys.executable, "-m", "tests.test_gpu_unit_real", out], cwd=root, env=env, check=True, timeout=120)
    off = np.load(out)
    on = group_states()
    assert sorted(off.files) == sorted(on) and len(on) == 32
    worst = max(float(np.max(np.abs(on[k] - off[k]))) for k in on)
    # (and the switch did something: the lists hold records the lowering rewrites)
    assert all(planner.lower_images(planner.plan_ops(n, group_lists(n, "none", 0)))[1] > 0 for n in SIZES)
    print(f"max |lowering on - lowering off| over the 32 group lists: {worst:.3e}")
    assert worst <= 1e-14


def test_random_circuit_through_the_searching_engine():
    """The 40-layer random 1q + CX circuit at 13 qubits through SingleGpuEngine with the layout search on: rewrite,
    priced planning, placement, lowering, device -- against the dense oracle."""
    from quantum_simulations_amd.circuit.io import validate_circuit_dict
    from quantum_simulations_amd.circuits import random_1q_cx_circuit
    from quantum_simulations_amd.runner.engine import SingleGpuEngine, gate_ops
    n = 13
    cd = validate_circuit_dict(random_1q_cx_circuit(n, depth=40))
    eng = SingleGpuEngine(n, layout="search")
    eng.LAYOUT_MIN_QUBITS = min(n, eng.LAYOUT_MIN_QUBITS)
    eng.init_zero_state()
    plan = eng.plan(cd)
    lowered = sum(planner.lower_images(planner.plan_ops(n, ops, masks, place))[1]
                  for ops, masks, place in zip(plan, plan.tiles, plan.placed or [None] * len(plan)))
    eng.execute(plan)
    got = eng.state_vector()
    eng.close()
    want = np.zeros(1 << n, dtype=np.complex128)
    want[0] = 1.0
    orc.apply_ops(want, gate_ops(cd))
    err = float(np.max(np.abs(got - want)))
    print(f"13 qubits, depth 40: {lowered} OPC_UNIT1 records in the plan, max |device - oracle| {err:.3e}")
    assert lowered >= 20
    assert err <= 1e-12


if __name__ == "__main__":             # the child of test_lowering_on_against_off: python -m tests.test_gpu_unit_real OUT.npz
    import sys
    np.savez(sys.argv[1], **group_states())
