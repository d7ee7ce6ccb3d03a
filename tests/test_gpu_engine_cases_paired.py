"""Every FULL gate case of the fused-pass engine as the SECOND tile of a workgroup, one test per case.

From 2 x 4096 tiles on (24 qubits with 11-bit tiles) a workgroup of k_tile takes two tiles (csrc/tile_launch.h,
`qsim_tiles_per_workgroup`): the gate engine runs twice per wave, the second tile's amplitudes are loaded before the
first run and stay live across it, the second run starts from the registers, EXEC / VCC and LDS contents the first one
left, and `baseh` -- what the outer predicates test -- is per tile.  tests/test_gpu_engine_cases.py runs its lists at 8
to 14 qubits: always one tile per workgroup.  Here the paired lists of tests/engine_cases.py (the FULL lists at 24 qubits
with the outer predicates on index bit 11, which differs INSIDE a tile pair, and on bit 23, which differs across the
grid; tests/test_engine_case_ledger.py proves on the CPU what each plan holds) run on a stand-alone 24-qubit chunk
(256 MiB: the cached instantiation) and on a 24-qubit view of a 512 MiB allocation (the streaming one).

State and reference.  The lists touch index bits 0..11 and 23 only, a 13-qubit active register; bits 12..22 look on.
The input is the product  psi0[b23, s, low] = chi[b23, low] * phi[s]  of a random 13-qubit state chi (a fixed seed
per case) and one fixed random unit vector phi of 2^11 distinct entries, so the expected state is the product of
phi with the extended-precision reference of the list on chi (bit 23 relabelled 12) -- exact, and milliseconds instead
of a 2^24 reference per case.  The two tiles of a workgroup differ in bit 11, inside chi; workgroups differ in phi
and in bit 23: every tile holds different data.  The outer product and the comparison are made in complex128: that
rounds amplitudes of at most 2e-3 to 1e-18.

Bounds: ATOL_KERNEL = 1e-12 (test_gpu_kernels.py: one kernel call on a normalised state with |matrix entries| <= 1)
for the one-pass lists; 1e-11, the bound of test_fused_tile_passes_vs_oracle for 90-op lists, for the three
multi-group lists; the two instantiations run the same arithmetic (the same assembly text, another cache policy of
the loads and stores), so their downloads are equal bit for bit.

Largest |device - reference| seen on an MI355X: see the CHANGELOG entry (per family, cached and streaming)."""
import numpy as np
import pytest

from tests import engine_cases as ec
from tests import tile_interpreter as ti
from tests.test_gpu_kernels import ATOL_KERNEL, _random_ops, _streaming_counts

pytestmark = pytest.mark.gpu

CASES = ec.paired_lists()
_SEED = {ec.case_id(c): i for i, c in enumerate(CASES)}      # one fixed random state per list
N, ACTIVE = ec.PAIRED_N, ec.PAIRED_ACTIVE
_SPECTATORS = N - ACTIVE                                     # index bits 12..22
MULTI_SEEDS = (650, 651, 652)                                # (the 13-qubit lists of test_fused_tile_passes_vs_oracle)
ATOL_MULTI = 1e-11


def multi_group_lists() -> list:
    """Three random 90-op lists on the 13 active qubits with qubit 12 relabelled 23: several passes of several register
    groups, merged phase runs, sunk swaps, mux pairs (planned on the CPU: tests/test_engine_case_ledger.py)."""
    return [[([23 if q == 12 else q for q in qubits], U) for qubits, U in _random_ops(ACTIVE, 90, seed)] for seed in MULTI_SEEDS]


def _spectator_vector() -> np.ndarray:
    rng = np.random.default_rng(20241)
    v = rng.standard_normal(1 << _SPECTATORS) + 1j * rng.standard_normal(1 << _SPECTATORS)
    return (v / np.linalg.norm(v)).astype(np.complex128)


def product_state(chi: np.ndarray, phi: np.ndarray) -> np.ndarray:
    """The top qubit of chi above phi's, its others below: chi on index bits 0..11 and 23, phi on bits 12..22 (complex128)."""
    chi = np.asarray(chi).astype(np.complex128)
    return (chi.reshape(2, 1, chi.size // 2) * phi.reshape(1, -1, 1)).reshape(-1)


@pytest.fixture(scope="module")
def chunks():
    """The two 24-qubit chunks every case runs on, the spectator vector, and `err`: the largest error per family."""
    from quantum_simulations_amd.kernel import planner
    from quantum_simulations_amd.kernel.device import DeviceChunk, device_count
    assert device_count() >= 1
    # the launch rule, which launch_tile itself calls: these chunks run two tiles per workgroup
    assert planner.tiles_per_workgroup(N, 11, 0) == 2
    lone = DeviceChunk.empty(N)                              # 256 MiB: not above the Infinity Cache, cached loads / stores
    parent = DeviceChunk.empty(N + 1)                        # 512 MiB: its views stream
    parent.init_zero(False)
    view = parent.view(1 << N, N)
    err = {}
    yield {"cached": lone, "streaming": view}, _spectator_vector(), err
    for key, worst in sorted(err.items()):
        print(f"\npaired engine-case max |device - reference| {key[0]:9s} {key[1]:10s} {worst:.3e}", end="")
    print()
    view.close()
    parent.close()
    lone.close()


def _run_both(held, psi0, want, ops, n_images, err, family, atol, what):
    got = {}
    for name, dev in held.items():
        dev.upload(psi0)
        dev.profile_begin()
        passes = dev.apply_ops(ops, fused=True)
        entries = dev.profile_end()
        launches, streamed = _streaming_counts(entries)
        got[name] = dev.download()
        worst = float(np.max(np.abs(got[name] - want)))
        print(f"{what} [{name}]: max |device - reference| = {worst:.3e}, passes {passes}")
        err[(name, family)] = max(err.get((name, family), 0.0), worst)
        assert passes == n_images
        assert [e["kernel"].startswith("k_tile") for e in entries if e["launches"]] == [True], entries
        assert launches == passes and streamed == (passes if name == "streaming" else 0), (name, launches, streamed)
        assert worst <= atol, (what, name)
    assert np.array_equal(got["cached"].view(np.uint64), got["streaming"].view(np.uint64)), what


@pytest.mark.parametrize("c", CASES, ids=ec.case_id)
def test_engine_case_paired(chunks, c):
    held, phi, err = chunks
    chi = ec.random_state(ACTIVE, 15000 + _SEED[ec.case_id(c)])
    want = product_state(ec.reference(chi, ec.to_active(c.ops)), phi)
    n_images = len(ti.plan(N, c.ops))
    assert n_images == 1
    _run_both(held, product_state(chi, phi), want, c.ops, n_images, err, c.family, ATOL_KERNEL, ec.case_id(c))


@pytest.mark.parametrize("which", range(len(MULTI_SEEDS)), ids=[f"seed{s}" for s in MULTI_SEEDS])
def test_multi_group_lists_paired(chunks, which):
    """Group changes through LDS, merged phase runs, sunk swaps and mux pairs as a second tile: 2 to 4 passes of several
    register groups each, against the dense oracle on the active register."""
    from oracle import dense_oracle
    held, phi, err = chunks
    ops = multi_group_lists()[which]
    chi = ec.random_state(ACTIVE, 16000 + which)
    small = chi.copy()
    dense_oracle.apply_ops(small, ec.to_active(ops))
    n_images = len(ti.plan(N, ops))
    assert n_images >= 2
    _run_both(held, product_state(chi, phi), product_state(small, phi), ops, n_images, err, "multi-group", ATOL_MULTI,
              f"multi-group seed {MULTI_SEEDS[which]}")
