"""Host side of shot sampling, no GPU: qsim_sample_locate (the block and local threshold of every uniform, a pure function
of the block prefix) against a numpy restatement, and quantum_simulations_amd/sampling.py (uniforms, layouts, marginals,
counts)."""
import ctypes as C

import numpy as np
import pytest

from quantum_simulations_amd import _lib, sampling
from quantum_simulations_amd.circuit.staging import permute_state
from quantum_simulations_amd.kernel.device import sample_block_bits, sample_locate

LAST = np.nextafter(1.0, 0.0)


def locate_ref(cdf, randnums):
    """searchsorted(C, r * total, 'right'), then back over zero-weight blocks; local threshold r * total - C[b - 1]."""
    cdf = np.asarray(cdf, dtype=np.float64)
    t = np.asarray(randnums, dtype=np.float64) * cdf[-1]
    weight = np.diff(np.concatenate([[0.0], cdf]))
    block = np.searchsorted(cdf, t, side="right")
    for s in range(len(block)):
        b = min(int(block[s]), len(cdf) - 1)
        while weight[b] == 0:
            b -= 1
        block[s] = b
    before = np.concatenate([[0.0], cdf])[block]
    return block.astype(np.uint64), t - before


def _check(cdf, randnums):
    block, local = sample_locate(cdf, randnums)
    want_block, want_local = locate_ref(cdf, randnums)
    assert block.dtype == np.uint64 and np.array_equal(block, want_block)
    assert np.array_equal(local, want_local) and np.all(local >= 0)
    weight = np.diff(np.concatenate([[0.0], np.asarray(cdf, dtype=np.float64)]))
    assert np.all(weight[block.astype(np.int64)] > 0)           # a zero-weight block is never chosen
    return block, local


EDGES = [0.0, -0.0, LAST, 0.5, 0.25, 0.75]


def test_block_bits():
    assert sample_block_bits() == 12


def test_locate_one_block():
    block, local = _check([2.5], EDGES)
    assert np.all(block == 0) and local[0] == 0.0 and local[2] == LAST * 2.5


@pytest.mark.parametrize("weights", [
    [0, 0, 1.0, 2.0],                      # zero-weight blocks at the start
    [1.0, 0, 0, 2.0, 0, 0.5],              # in the middle
    [1.0, 2.0, 0, 0],                      # at the end
    [0, 0.3, 0, 0, 0.7, 0, 0],             # everywhere
    [0, 0, 0, 4.0],                        # all the weight in the last block
])
def test_locate_zero_weight_blocks(weights):
    cdf = np.cumsum(np.asarray(weights, dtype=np.float64))
    block, _ = _check(cdf, EDGES + list(np.linspace(0, 1, 41, endpoint=False)))
    assert block[0] == np.flatnonzero(weights)[0]               # r = 0: the first block with weight
    assert block[2] == np.flatnonzero(weights)[-1]              # r = nextafter(1, 0): the last block with weight


def test_locate_threshold_on_a_prefix_value():
    cdf = np.array([1.0, 1.0, 2.0, 4.0, 4.0])                   # total 4: r = 0.25, 0.5 fall exactly on C[0] = C[1], C[2]
    block, local = _check(cdf, [0.25, 0.5, np.nextafter(0.25, 0), np.nextafter(0.5, 0)])
    assert list(block) == [2, 3, 0, 2] and local[0] == 0.0 and local[1] == 0.0


def test_locate_largest_uniform_stays_in_the_last_block_with_weight():
    # r = nextafter(1, 0) times the total stays below the total for every total (so the clamp to the last block with
    # weight is a guard, not a path a valid uniform takes), and lands in the last block that has weight
    for total in (1.0, 1.0 + 2.0 ** -52, 1.9, 3.0, 2.0 - 2.0 ** -52, 1e-300, 1e300):
        assert LAST * total < total
        block, local = _check(np.array([0.5 * total, total, total]), [LAST])
        assert block[0] == 1 and local[0] == LAST * total - 0.5 * total


def test_locate_random_shots():
    rng = np.random.default_rng(11)
    weights = rng.random(300) * (rng.random(300) > 0.3)
    weights[[0, 299]] = 0.0
    cdf = np.cumsum(weights)
    block, _ = _check(cdf, rng.random(10_000))
    assert len(np.unique(block)) > 100


@pytest.mark.parametrize("bad", [1.0, np.nan, -1e-300, np.inf, 1.5])
def test_locate_refuses_invalid_randnums(bad):
    with pytest.raises(ValueError, match="outside"):
        sample_locate([1.0, 2.0], [0.5, bad])
    sample_locate([1.0, 2.0], [-0.0])                           # -0.0 is valid


def test_locate_refuses_null_and_zero_total():
    lib = _lib.load()
    out_b, out_l, r, cdf = (C.c_uint64 * 1)(), (C.c_double * 1)(), (C.c_double * 1)(0.5), (C.c_double * 2)(0.0, 0.0)
    assert lib.qsim_sample_locate(2, cdf, 1, r, out_b, out_l) == _lib.QSIM_ERR_INVALID and lib.qsim_last_error()
    cdf[1] = 1.0
    assert lib.qsim_sample_locate(2, cdf, 1, r, out_b, out_l) == _lib.QSIM_OK
    assert lib.qsim_sample_locate(2, cdf, 1, r, None, out_l) == _lib.QSIM_ERR_INVALID
    assert lib.qsim_sample_locate(2, None, 1, r, out_b, out_l) == _lib.QSIM_ERR_INVALID
    assert lib.qsim_sample_locate(0, cdf, 1, r, out_b, out_l) == _lib.QSIM_ERR_INVALID


# ---- sampling.py
def test_draw_is_reproducible_and_is_pcg64():
    a, b = sampling.draw(1000, seed=5), sampling.draw(1000, seed=5)
    assert np.array_equal(a, b) and a.dtype == np.float64 and np.all((a >= 0) & (a < 1))
    assert not np.array_equal(a, sampling.draw(1000, seed=6))
    assert np.array_equal(a, np.random.Generator(np.random.PCG64(5)).random(1000))
    assert np.array_equal(sampling.draw(10, 5), a[:10])         # the first shots of a longer run
    assert sampling.draw(0).size == 0


@pytest.mark.parametrize("l2p", [[0, 1, 2, 3, 4], [4, 3, 2, 1, 0], [2, 0, 4, 1, 3], [1, 0, 2, 4, 3]])
def test_to_logical_agrees_with_permute_state_on_basis_states(l2p):
    n = len(l2p)
    got = sampling.to_logical(np.arange(1 << n, dtype=np.uint64), l2p)
    for i in range(1 << n):
        psi = np.zeros(1 << n, dtype=np.complex128)
        psi[i] = 1.0                                            # the PHYSICAL basis state i
        assert int(np.flatnonzero(permute_state(psi, l2p))[0]) == int(got[i])
    assert got.dtype == np.uint64 and sorted(got) == list(range(1 << n))


def test_to_logical_identity_and_hand_written():
    x = np.array([0, 5, 7], dtype=np.uint64)
    assert np.array_equal(sampling.to_logical(x), x) and sampling.to_logical(x) is not x
    # qubit 0 on bit 2, qubit 1 on bit 0, qubit 2 on bit 1: index 0b001 -> qubit 1 set -> 0b010
    assert list(sampling.to_logical([0b001, 0b100, 0b110], [2, 0, 1])) == [0b010, 0b001, 0b101]
    big = np.array([1 << 40], dtype=np.uint64)
    l2p = list(range(41))
    l2p[0], l2p[40] = 40, 0
    assert int(sampling.to_logical(big, l2p)[0]) == 1


def test_marginal_hand_written():
    assert list(sampling.marginal([0b1010, 0b0110, 0b0001], [1, 3])) == [0b11, 0b01, 0b00]
    assert list(sampling.marginal([0b1010, 0b0110, 0b0001], [3, 1])) == [0b11, 0b10, 0b00]
    assert list(sampling.marginal([0b1010], [0])) == [0] and sampling.marginal([3], [0]).dtype == np.uint64
    with pytest.raises(ValueError):
        sampling.marginal([1], [0, 0])


def test_counts_hand_written():
    assert sampling.counts([0, 3, 3, 4, 0, 0], 3) == {"000": 3, "011": 2, "100": 1}
    assert sampling.counts([1], 2) == {"01": 1}                 # qubit 0 is the RIGHTMOST character
    assert sampling.counts([], 4) == {}
    assert sum(sampling.counts(sampling.draw(500, 1) < 0.5, 1).values()) == 500
    with pytest.raises(ValueError):
        sampling.counts([8], 3)


def test_engine_modules_export_sample_next_to_expectation():
    from quantum_simulations_amd.runner import single_node
    from quantum_simulations_amd.runner.engine import SingleGpuEngine
    assert callable(single_node.sample) and callable(single_node.expectation)
    assert callable(SingleGpuEngine.sample) and callable(SingleGpuEngine.expectation)
