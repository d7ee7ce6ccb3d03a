"""Cyclic plans on the device (`qsim_cycle_create`, `qsim_apply_cycle`, `device.Cycle`, the deferred tail of
csrc/abi_pending.h): one execution of an op list L = A.B runs the head A -- or B.A when the cycle's tail is deferred on the
chunk -- and leaves the tail B deferred; NOBODY may see a state with the tail missing.  Sizes: 12 qubits (the first with more
than one tile), 14 (more than one pass), 24 (the first where a workgroup takes two tiles).  Cycles are hand-made, the tail
being the last m ops of L for m = 1, a tenth of the list and half of it (a product of L whatever m is).  Three applications
with nothing in between, then with a norm2 after the first, a fingerprint after the second, a plain apply_ops of one gate in
between, and a second cycle object alternating with the first: every variant must give the state that the plain lists
applied in that order give -- at 12 and 14 qubits the download against oracle/dense_oracle.py at 1e-12, at 24 qubits the
fingerprint against the plain `apply_ops` path at bench.py's PARITY_TOL (1e-10).  `init_zero` drops a deferred tail
(|0..0> stays |0..0>), and destroying chunk and cycle in either order is clean."""
import functools

import numpy as np
import pytest

from oracle import dense_oracle as orc
from quantum_simulations_amd.kernel import planner
from tests.test_gpu_kernels import ATOL_KERNEL, _rand_state, _rand_unitary

pytestmark = pytest.mark.gpu

PARITY_TOL = 1e-10                     # bench.py PARITY_TOL
SIZES = (12, 14, 24)
SHARES = ("one", "tenth", "half")
FP_SEED = 20260504


@functools.lru_cache(maxsize=None)
def _ops(n):
    from quantum_simulations_amd.circuit.io import validate_circuit_dict
    from quantum_simulations_amd.circuits import random_1q_cx_circuit
    from quantum_simulations_amd.runner.engine import gate_ops
    return planner.rewrite_ops(n, gate_ops(validate_circuit_dict(random_1q_cx_circuit(n, depth=40 if n < 20 else 12, seed=n))))


def _other(n):
    """a second op list: the first one backwards"""
    return _ops(n)[::-1]


def _gate(n):
    return [([n - 2], _rand_unitary(2, 5))]


def _tail_ops(ops, share):
    return {"one": 1, "tenth": max(2, len(ops) // 10), "half": len(ops) // 2}[share]


def _cycle(n, ops, share):
    from quantum_simulations_amd.kernel.device import Cycle
    m = _tail_ops(ops, share)
    head, tail = ops[:-m], ops[-m:]
    return Cycle(n, (head, None, None), (tail + head, None, None), (tail, None, None))


# a variant: the calls on the chunk in order -- "L" / "M": one execution of the first / second list (through its cycle, or
# plain), "norm2" / "fp": a readout in between (its value must be the plain path's too), "gate": a plain apply_ops of one gate
VARIANTS = {
    "thrice": ("L", "L", "L"),
    "readouts": ("L", "norm2", "L", "fp", "L"),
    "gate": ("L", "gate", "L", "L"),
    "two_cycles": ("L", "M", "L", "M"),
}


def _play(dev, n, steps, run):
    seen = []
    for step in steps:
        if step == "norm2":
            seen.append(dev.norm2())
        elif step == "fp":
            seen.append(dev.fingerprint(n, 0, None, FP_SEED))
        elif step == "gate":
            dev.apply_ops(_gate(n))
        else:
            run(step)
    return seen


@pytest.fixture(scope="module")
def chunks():
    from quantum_simulations_amd.kernel.device import DeviceChunk, device_count
    assert device_count() >= 1
    held = {n: DeviceChunk.empty(n) for n in SIZES}
    yield held
    for dev in held.values():
        dev.close()


@pytest.fixture(scope="module")
def plain(chunks):
    """what the plain lists give, once per (size, variant): the oracle's state (12, 14 qubits) or the device's fingerprint
    of the plain `apply_ops` path (24), and the readouts on the way"""
    @functools.lru_cache(maxsize=None)
    def of(n, variant):
        lists = {"L": _ops(n), "M": _other(n)}
        if n < 20:
            psi = _rand_state(n, n).copy()
            seen = []
            for step in VARIANTS[variant]:
                if step == "norm2":
                    seen.append(float(np.vdot(psi, psi).real))
                elif step == "fp":
                    seen.append(None)              # (checked at 24 qubits, where the plain path runs on the device)
                else:
                    orc.apply_ops(psi, _gate(n) if step == "gate" else lists[step])
            psi.setflags(write=False)
            return psi, seen
        dev = chunks[n]
        dev.init_random(n)
        seen = _play(dev, n, VARIANTS[variant], lambda step: dev.apply_ops(lists[step]))
        return dev.fingerprint(n, 0, None, FP_SEED), seen
    return of


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("share", SHARES)
@pytest.mark.parametrize("n", SIZES)
def test_cycles_give_what_the_plain_lists_give(chunks, plain, n, share, variant):
    want, want_seen = plain(n, variant)
    dev = chunks[n]
    cycles = {"L": _cycle(n, _ops(n), share), "M": _cycle(n, _other(n), share)}
    if n < 20:
        dev.upload(_rand_state(n, n))
    else:
        dev.init_random(n)
    launched = []
    seen = _play(dev, n, VARIANTS[variant], lambda step: launched.append(dev.apply_cycle(cycles[step])))
    for got, ref in zip(seen, want_seen):
        if ref is not None:
            assert abs(got - ref) < PARITY_TOL, (got, ref)
    if n < 20:
        err = float(np.max(np.abs(dev.download() - want)))
        bound = ATOL_KERNEL
    else:
        err = abs(dev.fingerprint(n, 0, None, FP_SEED) - want)
        bound = PARITY_TOL
    print(f"n {n}, tail {_tail_ops(_ops(n), share)} of {len(_ops(n))} ops, {variant}: passes (head, steady, tail) "
          f"{cycles['L'].passes}, launched {launched}, |cycle - plain| {err:.3e}")
    # steady passes exactly where the same cycle's tail is still deferred: any other call on the chunk has settled it
    expected, deferred = [], None
    for step in VARIANTS[variant]:
        if step in cycles:
            expected.append(cycles[step].passes[1 if deferred == step else 0])
        deferred = step if step in cycles else None
    assert launched == expected
    assert err <= bound
    for c in cycles.values():
        c.close()


@pytest.mark.parametrize("n", SIZES)
def test_init_zero_drops_the_tail_and_destroy_is_clean(n):
    from quantum_simulations_amd.kernel.device import DeviceChunk
    dev = DeviceChunk.zero_state(n)
    cycle = _cycle(n, _ops(n), "half")
    dev.apply_cycle(cycle)
    dev.apply_cycle(cycle)
    dev.init_zero(True)                                   # (the tail of the second application must not run after this)
    if n < 20:
        psi = dev.download()
        assert psi[0] == 1.0 and not np.any(psi[1:])
    else:
        assert dev.count_nonzero(0.0) == 1 and abs(dev.norm2() - 1.0) < 1e-15
    dev.apply_cycle(cycle)
    cycle.close()                                         # (the cycle goes first: the deferred tail keeps its passes)
    n2 = dev.norm2()
    assert abs(n2 - 1.0) < 1e-12
    other = _cycle(n, _ops(n), "tenth")
    dev.apply_cycle(other)
    dev.close()                                           # (the chunk goes with a tail deferred)
    other.close()


def test_views_and_wrapped_chunks_cannot_defer_a_tail():
    from quantum_simulations_amd.kernel.device import DeviceChunk
    n = 12
    dev = DeviceChunk.zero_state(n + 1)
    view = dev.view(0, n)
    cycle = _cycle(n, _ops(n), "tenth")
    with pytest.raises(ValueError, match="own its memory"):
        view.apply_cycle(cycle)
    # ... and a view sees its parent's tail: the parent's cycle, then a read through a view of the same amplitudes
    whole = _cycle(n + 1, [(qs, U) for qs, U in _ops(n)], "half")
    psi = _rand_state(n + 1, 3)
    dev.upload(psi)
    dev.apply_cycle(whole)
    got = np.concatenate([view.download(), dev.view(1 << n, n).download()])
    orc.apply_ops(psi, _ops(n))
    assert float(np.max(np.abs(got - psi))) <= ATOL_KERNEL
    for c in (cycle, whole):
        c.close()
    view.close()
    dev.close()


def test_the_engine_runs_its_cyclic_finalists():
    """`SingleGpuEngine.finalist_plans` for 8 executions at 14 qubits: the cyclic finalists (one layout for three lists,
    each priced and placed) executed three times from |0..0>, compared through the layout with the oracle's L.L.L; the
    launches are head, steady, steady, and the plain finalists stay next to them; with CYCLES off there are none."""
    from quantum_simulations_amd.circuit.fusion import batch_levels
    from quantum_simulations_amd.circuit.io import levelize, validate_circuit_dict
    from quantum_simulations_amd.circuits import random_1q_cx_circuit
    from quantum_simulations_amd.runner.engine import SingleGpuEngine, gate_ops
    n = 14
    cd = validate_circuit_dict(random_1q_cx_circuit(n, depth=40, seed=n))
    want = np.zeros(1 << n, dtype=np.complex128)
    want[0] = 1.0
    for _ in range(3):
        orc.apply_ops(want, gate_ops(cd))
    batches = [p["local_ops"] for p in batch_levels(levelize(cd), n)]
    eng = SingleGpuEngine(n, layout="search")
    eng.LAYOUT_MIN_QUBITS = min(n, eng.LAYOUT_MIN_QUBITS)
    try:
        plans = eng.finalist_plans(batches, eng.LAYOUT_FINALISTS, repeats=eng.LAYOUT_MIN_REPEATS)
        cyclic = [p for p in plans if p.cycle is not None]
        assert cyclic and len(cyclic) < len(plans)
        for plan in cyclic:
            passes = plan.layout_info["cycle_passes"]
            assert passes["steady"] < passes["plain"] and plan.layout_info["passes_chosen"] == passes["steady"]
            eng.init_zero_state()
            launched = []
            for _ in range(3):
                eng.execute(plan)
                launched.append(eng.passes_per_step(plan))
            err = float(np.max(np.abs(eng.state_vector() - want)))
            print(f"line qubits {plan.layout_info['line_qubits']}: {passes}, launched {launched}, max |device - oracle| {err:.3e}")
            assert launched == [passes["head"], passes["steady"], passes["steady"]]
            assert err <= ATOL_KERNEL
        eng.CYCLES = False
        assert all(p.cycle is None for p in eng.finalist_plans(batches, eng.LAYOUT_FINALISTS, repeats=eng.LAYOUT_MIN_REPEATS))
    finally:
        eng.close()
