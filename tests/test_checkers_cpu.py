"""The CPU side of the checker tests (tests/test_gpu_checkers.py has the device side).

A non-finite amplitude on ONE rank must show on EVERY rank: `closed_form_error` and `closed_form_sample_error` of the
multi-GPU engine's checks (runner/distributed_checks.py) turn a non-finite local value into +inf before the maximum over
ranks, because what a MAX reduction (and Python's `max`) does with a NaN is not defined.  Two gloo ranks over the numpy
test double, the GHZ state, one NaN planted in the last amplitude of the last rank's shard.

And what the device tests rest on: the launch constants they derive their edge indices from are the ones in the sources,
and the numpy restatement of the random fill is the documented formula."""
import os
import sys
import traceback
from pathlib import Path

import numpy as np

from tests import checker_reference as ref
from tests.test_distributed_gloo import _spawn

ROOT = Path(__file__).resolve().parent.parent


def _nan_worker(rank, world, port, errors):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
        sys.path.insert(0, str(ROOT))
        from quantum_simulations_amd import circuits as gen
        from quantum_simulations_amd.runner.distributed import DistributedEngine
        from tests.cpu_shard_backend import CpuShardBackend
        n = 6
        k = n - (world.bit_length() - 1)
        eng = DistributedEngine(n, world, rank, backend=CpuShardBackend(k), staging=False, min_piece_qubits=1)
        eng.init_zero_state()
        eng.execute(eng.plan(gen.generate_ghz_circuit(n)))
        checks = (lambda: eng.closed_form_error("ghz"),
                  lambda: eng.closed_form_sample_error("ghz", windows=5, window=8))   # (the last window ends the shard)
        for check in checks:
            assert check() < 1e-12
        st = eng.backend._c("state")
        nan = float("nan")
        for bad in (complex(nan, 0.0), complex(0.0, nan), complex(nan, nan), complex(float("inf"), 0.0)):
            saved = complex(st[-1])
            if rank == world - 1:
                st[-1] = bad
            for check in checks:
                err = check()                           # collective: every rank asks, every rank must be told
                assert not np.isfinite(err), (rank, bad, err)
                assert not err < 1e-10, (rank, bad, err)
            st[-1] = saved
            for check in checks:
                assert check() < 1e-12, (rank, bad)
        eng.close()
    except Exception:
        errors.put((rank, traceback.format_exc()))
        raise


def test_a_non_finite_amplitude_on_one_rank_shows_on_every_rank():
    _spawn(_nan_worker, 2)


def test_launch_constants_are_the_ones_in_the_sources():
    """The edge indices of the device tests straddle the grid stride of each kernel; a changed constant moves the stride."""
    csrc = ROOT / "quantum_simulations_amd" / "csrc"
    assert f"constexpr int kBlock = {ref.K_BLOCK};" in (csrc / "gate_kernels.h").read_text()
    readout = (csrc / "readout_kernels.h").read_text()
    assert f"constexpr int kReduceBlocks = {ref.K_REDUCE_BLOCKS};" in readout
    assert f"std::max<u64>(want, 1), {ref.STREAM_GRID_MAX});" in (csrc / "state_kernels.h").read_text()
    abi = (csrc / "abi_readout.h").read_text()
    assert abi.count("std::min<unsigned>(stream_grid(amps(c)), kReduceBlocks);") == 2       # the norm and the closed form
    assert abi.count("std::min<unsigned>(stream_grid(amps(c)), kReduceBlocks / 2);") == 1   # the fingerprint
    assert (ref.T_REDUCE, ref.T_FINGERPRINT, ref.T_STREAM) == (1 << 19, 1 << 18, 1 << 21)


def test_edge_indices_straddle_the_stride():
    got = ref.edge_indices(21, ref.T_REDUCE)
    for i in (0, 63, 64, 255, 256, (1 << 19) - 1, 1 << 19, (1 << 19) + 255, (1 << 20) - 1, (1 << 21) - 1):
        assert i in got
    assert got == sorted(set(got)) and 10 < len(got) <= 18 and got == ref.edge_indices(21, ref.T_REDUCE)
    assert ref.edge_indices(1, ref.T_REDUCE) == [0, 1]
    assert max(ref.edge_indices(19, ref.T_REDUCE)) == (1 << 19) - 1


def test_random_fill_restatement_is_the_documented_formula():
    """u(j) = (fp_mix(seed + j) >> 11) * 2^-52 - 1 in Python integers (exact), seed + j wrapping at 2^64."""
    m64 = (1 << 64) - 1

    def mix(x):
        x = (x + 0x9E3779B97F4A7C15) & m64
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & m64
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & m64
        return x ^ (x >> 31)
    for seed in (0, 7, 2 ** 64 - 12345):
        first = 12340 if seed > 7 else 3
        got = ref.random_fill_uniforms(seed, first, 16)
        want = [float((mix((seed + j) & m64) >> 11) - (1 << 52)) / float(1 << 52) for j in range(first, first + 16)]
        assert got.tolist() == want
        assert np.all((got >= -1.0) & (got < 1.0))
    amps = ref.random_fill_amplitudes(7, 4)
    assert amps.shape == (16,) and abs(np.vdot(amps, amps).real - 1.0) < 1e-15
    assert ref.bit_equal(ref.random_fill_amplitudes(7, 4, 5, 3), amps[5:8])
