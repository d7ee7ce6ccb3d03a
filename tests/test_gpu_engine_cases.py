"""Every gate case of the fused-pass engine on the device, one test per case.

Each directed op list of tests/engine_cases.py is aimed at one (engine text, family, variant, predicate form) of the
engine's branch table -- the test id names it, tests/test_engine_case_ledger.py proves on the CPU that the planned
pass holds it.  Here the list runs through `qsim_apply_ops` on a structureless random state and the result is
compared with the gate-by-gate np.longdouble reference at the per-kernel-call bound of test_gpu_kernels.py
(ATOL_KERNEL = 1e-12 absolute: one pass on a normalised state with |matrix entries| <= 1).  The pass count the
device reports equals the number of images `qsim_plan_ops` gives for the list, so the device ran the plan the
ledger inspected.  The FULL lists of 14 qubits run once more on a view inside a 512 MiB allocation: the streaming
(non-temporal) instantiation of k_tile.

Largest |device - reference| seen on an MI355X over all lists: 4.5e-17 (the CHANGELOG entry has it per family)."""
import numpy as np
import pytest

from tests import engine_cases as ec
from tests import tile_interpreter as ti
from tests.test_gpu_kernels import ATOL_KERNEL, _streaming_counts

pytestmark = pytest.mark.gpu

CASES = ec.directed_lists()
STREAMING_CASES = [c for c in CASES if c.text == ec.FULL and c.n == 14]
_SEED = {ec.case_id(c): i for i, c in enumerate(CASES)}      # one fixed random state per list


@pytest.fixture(scope="module")
def chunks():
    """One device chunk per size, reused by every list of that size; `err` collects the largest error per family."""
    from quantum_simulations_amd.kernel.device import DeviceChunk, device_count
    assert device_count() >= 1
    sizes = sorted({c.n for c in CASES})
    held = {n: DeviceChunk.empty(n) for n in sizes}
    parent = DeviceChunk.empty(25)                           # 2^25 amplitudes = 512 MiB > the 256 MiB Infinity Cache
    parent.init_zero(False)
    held["view"] = parent.view(5 << 14, 14)
    err = {}
    yield held, err
    for key, worst in sorted(err.items()):
        print(f"\nengine-case max |device - reference| {key[0]:8s} {key[1]:10s} {worst:.3e}", end="")
    print()
    for n in sizes + ["view"]:
        held[n].close()
    parent.close()


def _run(dev, c, seed, err, key, streaming):
    psi0 = ec.random_state(c.n, seed)
    want = ec.reference(psi0, c.ops)
    n_images = len(ti.plan(c.n, c.ops))
    dev.upload(psi0)
    dev.profile_begin()
    passes = dev.apply_ops(c.ops, fused=True)
    launches, streamed = _streaming_counts(dev.profile_end())
    got = dev.download()
    worst = float(np.max(np.abs(got - want)))
    print(f"{ec.case_id(c)}: max |device - reference| = {worst:.3e}, passes {passes}")
    err[key] = max(err.get(key, 0.0), worst)
    assert passes == n_images == 1
    assert launches == passes and streamed == (passes if streaming else 0), (launches, streamed)
    assert worst <= ATOL_KERNEL, ec.case_id(c)


@pytest.mark.parametrize("c", CASES, ids=ec.case_id)
def test_engine_case(chunks, c):
    held, err = chunks
    _run(held[c.n], c, 5000 + _SEED[ec.case_id(c)], err, (c.text, c.family), streaming=False)


@pytest.mark.parametrize("c", STREAMING_CASES, ids=ec.case_id)
def test_engine_case_streaming(chunks, c):
    held, err = chunks
    _run(held["view"], c, 9000 + _SEED[ec.case_id(c)], err, ("FULL-nt", c.family), streaming=True)
