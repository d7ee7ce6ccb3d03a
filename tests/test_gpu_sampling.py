"""qsim_sample on an MI355X.  The acceptance criterion of every shot does not depend on the device's summation order: with
p = |amp|^2 and P = cumsum(p) of the downloaded state in numpy.longdouble, total = P[-1] and tol = 1e-12 * total (the
absolute tolerance of the other readout tests on norm-1 states), index i returned for uniform r is right iff

    P[i-1] - tol <= r * total <= P[i] + tol   and   p[i] > 0,

and no shot may fail.  Sizes: chunks below 256 amplitudes, around the block length 2^B (B = qsim_sample_block_bits()),
16 and 20 qubits; views; states with zero-weight blocks and zero-weight amplitudes; the engine and single_node paths in
non-identity layouts.  (The block prefix is scanned on the host, so there is no size at which a device scan changes form.)"""
import ctypes as C

import numpy as np
import pytest

from quantum_simulations_amd import _lib, sampling
from quantum_simulations_amd import circuits as gen
from quantum_simulations_amd.circuit.staging import permute_state
from quantum_simulations_amd.kernel.device import DeviceChunk, sample_block_bits

pytestmark = pytest.mark.gpu

B = 12
LAST = np.nextafter(1.0, 0.0)
RANDNUMS = np.concatenate([sampling.draw(2000, seed=17), [0.0, LAST, 0.5]])
SIZES = list(range(1, 9)) + [B - 1, B, B + 1, 16, 20]


def test_block_bits_is_what_the_sizes_assume():
    assert sample_block_bits() == B


def failures(psi, randnums, indices, device_total=None):
    """The shots that miss the criterion (empty = all right), from the state as downloaded."""
    re, im = psi.real.astype(np.longdouble), psi.imag.astype(np.longdouble)
    p = re * re + im * im
    P = np.cumsum(p)
    total = P[-1]
    tol = np.longdouble(1e-12) * total
    i = np.asarray(indices).astype(np.int64)
    assert i.shape == np.shape(randnums) and np.all((i >= 0) & (i < len(psi)))
    t = np.asarray(randnums).astype(np.longdouble) * total
    below = np.where(i > 0, P[np.maximum(i - 1, 0)], np.longdouble(0))
    ok = (below - tol <= t) & (t <= P[i] + tol) & (p[i] > 0)
    if device_total is not None:
        print(f"n={len(psi).bit_length() - 1} total {float(total)!r} device {device_total!r} "
              f"diff {float(abs(np.longdouble(device_total) - total)):.3e} tol {float(tol):.3e}")
        assert abs(np.longdouble(device_total) - total) <= tol
    return np.flatnonzero(~ok)


def _sample_checked(psi, randnums=RANDNUMS, chunk=None):
    c = chunk if chunk is not None else DeviceChunk.from_numpy(psi)
    try:
        assert np.array_equal(c.download(), psi)
        idx = c.sample(randnums)
        assert idx.dtype == np.uint64 and c.last_sample_passes == 2
        bad = failures(psi, randnums, idx, c.last_sample_total)
        assert bad.size == 0, (len(psi), bad[:5], idx[bad[:5]], np.asarray(randnums)[bad[:5]])
        again = c.sample(randnums)
        assert idx.tobytes() == again.tobytes()                      # two calls give the same bits
        return idx
    finally:
        if chunk is None:
            c.close()


def _random(n, seed):
    rng = np.random.default_rng(seed)
    return 1.9 * (rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)) / np.sqrt(2.0 ** (n + 1))


@pytest.mark.parametrize("n", SIZES)
def test_random_unnormalised_state(n):
    _sample_checked(_random(n, n))


@pytest.mark.parametrize("n", SIZES)
def test_ghz(n):
    psi = np.zeros(1 << n, dtype=np.complex128)
    psi[0] = psi[-1] = np.sqrt(0.5)
    idx = _sample_checked(psi)
    assert set(np.unique(idx)) == {0, (1 << n) - 1}
    assert idx[-3] == 0 and idx[-2] == (1 << n) - 1                  # r = 0, r = nextafter(1, 0)


@pytest.mark.parametrize("n", SIZES)
def test_support_only_where_the_top_bit_is_one(n):
    psi = _random(n, 40 + n)
    psi[: 1 << (n - 1)] = 0.0                                         # n > B: whole leading blocks have zero weight
    idx = _sample_checked(psi)
    assert np.all(idx >= (1 << (n - 1)))


@pytest.mark.parametrize("n", SIZES)
def test_support_only_where_bit_zero_is_zero(n):
    psi = _random(n, 60 + n)
    psi[1::2] = 0.0
    idx = _sample_checked(psi)
    assert np.all(idx & np.uint64(1) == 0)


@pytest.mark.parametrize("n", [B + 2, 16])
@pytest.mark.parametrize("where", ["last of block 1", "first of block 2"])
def test_basis_state_at_a_block_edge(n, where):
    at = (2 << B) - 1 if where == "last of block 1" else 2 << B
    psi = np.zeros(1 << n, dtype=np.complex128)
    psi[at] = 0.6 - 0.8j
    assert np.all(_sample_checked(psi) == at)


def test_many_shots_in_one_block():
    psi = np.zeros(1 << 16, dtype=np.complex128)
    psi[(5 << B) + 77] = 1j
    r = sampling.draw(1 << 16, seed=3)
    assert np.all(_sample_checked(psi, r) == (5 << B) + 77)
    two = np.zeros(1 << 16, dtype=np.complex128)                      # and two amplitudes of one block, 1/4 : 3/4
    two[(9 << B) + 1], two[(9 << B) + 4000] = 0.5, np.sqrt(0.75)
    assert set(np.unique(_sample_checked(two, r))) == {(9 << B) + 1, (9 << B) + 4000}


def test_more_shots_than_amplitudes():
    psi = _random(3, 5)
    r = sampling.draw(10_000, seed=8)
    idx = _sample_checked(psi, r)
    assert set(np.unique(idx)) == set(range(8))
    p = np.abs(psi) ** 2
    assert np.max(np.abs(np.bincount(idx.astype(np.int64), minlength=8) / 10_000 - p / p.sum())) < 0.02


def test_no_shots():
    c = DeviceChunk.from_numpy(_random(6, 1))
    try:
        out = c.sample([])
        assert out.size == 0 and out.dtype == np.uint64 and c.last_sample_passes == 0
        out = c.sample(np.empty(0))
        assert out.size == 0 and c.last_sample_passes == 0
    finally:
        c.close()


@pytest.mark.parametrize("n", [5, B + 1, 16])
def test_permuted_randnums_give_the_permuted_result(n):
    psi = _random(n, 80 + n)
    c = DeviceChunk.from_numpy(psi)
    try:
        first = c.sample(RANDNUMS)
        perm = np.random.default_rng(2).permutation(len(RANDNUMS))
        assert np.array_equal(c.sample(RANDNUMS[perm]), first[perm])
        assert np.array_equal(c.sample(RANDNUMS[:100]), first[:100])  # a shot does not depend on the others
    finally:
        c.close()


def test_views():
    psi = _random(14, 5)
    c = DeviceChunk.from_numpy(psi)
    try:
        for off in (0, 3 << 10, 15 << 10):
            v = c.view(off, 10)
            try:
                idx = v.sample(RANDNUMS)
                assert failures(psi[off: off + 1024], RANDNUMS, idx, v.last_sample_total).size == 0
            finally:
                v.close()
        v = c.view(1 << 13, 13)                                       # a view of two blocks
        try:
            assert failures(psi[1 << 13:], RANDNUMS, v.sample(RANDNUMS), v.last_sample_total).size == 0
        finally:
            v.close()
    finally:
        c.close()


def test_wrapped_memory():
    psi = _random(13, 9)
    owner = DeviceChunk.from_numpy(psi)
    try:
        w = DeviceChunk.wrap_pointer(owner.device_ptr, 13, owner.device, keep=owner)
        try:
            owner.sync()
            assert failures(psi, RANDNUMS, w.sample(RANDNUMS), w.last_sample_total).size == 0
        finally:
            w.close()
    finally:
        owner.close()


def test_errors():
    lib = _lib.load()
    c = DeviceChunk.from_numpy(_random(8, 1))
    try:
        with pytest.raises(ValueError, match="outside"):
            c.sample([0.5, 1.0])
        with pytest.raises(ValueError, match="outside"):
            c.sample([np.nan])
        c.sample([-0.0])
        r, out = np.full(4, 0.5), np.zeros(4, dtype=np.uint64)
        total, passes = C.c_double(), C.c_int()
        rp, op = _lib.ptr(r), _lib.ptr(out)
        assert lib.qsim_sample(c._h, (1 << 24) + 1, rp, op, C.byref(total), C.byref(passes)) == _lib.QSIM_ERR_INVALID
        assert b"2^24" in lib.qsim_last_error()
        assert lib.qsim_sample(c._h, 4, rp, None, C.byref(total), C.byref(passes)) == _lib.QSIM_ERR_INVALID
        assert b"null" in lib.qsim_last_error()
        assert lib.qsim_sample(c._h, 4, None, op, C.byref(total), C.byref(passes)) == _lib.QSIM_ERR_INVALID
        assert lib.qsim_sample(c._h, 4, rp, op, None, C.byref(passes)) == _lib.QSIM_ERR_INVALID
        assert lib.qsim_sample(c._h, 4, rp, op, C.byref(total), None) == _lib.QSIM_ERR_INVALID
        assert lib.qsim_sample(None, 4, rp, op, C.byref(total), C.byref(passes)) == _lib.QSIM_ERR_INVALID
        assert lib.qsim_sample(c._h, 4, rp, op, C.byref(total), C.byref(passes)) == _lib.QSIM_OK
    finally:
        c.close()
    z = DeviceChunk.zero_state(13, set_amp0=False)
    try:
        with pytest.raises(ValueError, match="nothing to sample"):
            z.sample([0.5])
    finally:
        z.close()


def _check_logical(psi_logical, l2p, values, shots, seed):
    """`values` = logical samples; the criterion on the state as it lies in memory, rebuilt from the LOGICAL state."""
    n = len(psi_logical).bit_length() - 1
    logical_of = sampling.to_logical(np.arange(1 << n, dtype=np.uint64), l2p).astype(np.int64)
    physical_of = np.argsort(logical_of)
    assert failures(psi_logical[logical_of], sampling.draw(shots, seed), physical_of[values.astype(np.int64)]).size == 0


def test_engine_in_a_non_identity_layout():
    from quantum_simulations_amd.runner.engine import SingleGpuEngine
    n = 14
    eng = SingleGpuEngine(n, layout="search")
    try:
        eng.LAYOUT_MIN_QUBITS = n                                     # search a layout for this small state too
        eng.init_zero_state()
        plan = eng.plan(gen.random_1q_cx_circuit(n, depth=6, seed=9), repeats=8)
        assert plan.l2p is not None and plan.l2p != list(range(n))    # the plan was written for a non-identity layout
        eng.execute(plan)
        assert eng.l2p == plan.l2p
        layouts = [eng.l2p, [int(p) for p in np.random.default_rng(3).permutation(n)]]
        print("planned layout", layouts[0])
        for l2p in layouts:
            if l2p is not layouts[0]:
                eng._adopt_layout(l2p)                                # (SWAP passes: the state now lives in that layout)
                assert eng.l2p == l2p and l2p != list(range(n))
            before = eng.state.download()
            values = eng.sample(2003, seed=4)
            assert values.dtype == np.uint64 and np.array_equal(eng.state.download(), before)   # read-only
            _check_logical(eng.state_vector(), eng.l2p, values, 2003, 4)
            assert np.array_equal(values, sampling.to_logical(eng.state.sample(sampling.draw(2003, 4)), eng.l2p))
            qubits = [n - 1, 0, 5]
            assert np.array_equal(eng.sample(2003, seed=4, qubits=qubits), sampling.marginal(values, qubits))
    finally:
        eng.close()


def test_single_node_staged():
    from quantum_simulations_amd.runner import single_node
    n = 12
    cd = gen.random_1q_cx_circuit(n, depth=8, seed=5)
    buf = single_node.run(cd, chunk_size=1 << 9, use_fusion=True, use_staging=True)
    try:
        assert buf.log_to_phys and buf.log_to_phys != list(range(n))
        psi = permute_state(single_node.collect_state(buf), buf.log_to_phys)
        values = single_node.sample(buf, 2003, seed=6)
        _check_logical(psi, buf.log_to_phys, values, 2003, 6)
        qubits = [3, 11, 0, 7]
        assert np.array_equal(single_node.sample(buf, 2003, seed=6, qubits=qubits), sampling.marginal(values, qubits))
        counts = sampling.counts(single_node.sample(buf, 2003, seed=6, qubits=[0]), 1)
        assert sum(counts.values()) == 2003 and set(counts) <= {"0", "1"}
    finally:
        buf.close()
