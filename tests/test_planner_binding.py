"""The Python binding of the host planner (kernel/planner.py), on the CPU: the pass image's layout is the kernel's, the
image buffer of `plan_ops` holds short and long plans alike, and searched tiles, the peeked pass and parallel callers get
what the library gives a direct call."""
import ctypes as C
import functools
import os
import re
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from quantum_simulations_amd import _lib
from quantum_simulations_amd.circuit.io import validate_circuit_dict
from quantum_simulations_amd.circuits import random_1q_cx_circuit
from quantum_simulations_amd.kernel import planner
from quantum_simulations_amd.kernel.device import pack_ops
from quantum_simulations_amd.runner.engine import gate_ops
from tests.test_tile_planner_cpu import _long_list_with_a_control_only_qubit


def _rand_ops(n, depth, seed):
    return gate_ops(validate_circuit_dict(random_1q_cx_circuit(n, depth=depth, seed=seed)))


@functools.lru_cache(maxsize=None)
def _lists():
    """(n, ops) of a plan that fits the first buffer of `plan_ops` and of one that does not"""
    return {"short": (14, _rand_ops(14, 40, 11)), "long": (28, _long_list_with_a_control_only_qubit(28, 4000, 1))}


def test_the_pass_image_is_the_kernel_argument_block():
    assert planner.PASS_IMAGE.itemsize == planner.IMAGE_BYTES == 4096
    assert [planner.PASS_IMAGE.fields[f][1] for f in ("T", "h", "stream")] == [12, 16, 192]
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "quantum_simulations_amd", "csrc", "tile_kernel.h")
    with open(header) as f:
        found = re.findall(r"constexpr\s+int\s+kTileStreamOff\s*=\s*(\d+)\s*;", f.read())
    assert [int(x) for x in found] == [192] and planner.STREAM_OFF == 192


def test_plan_ops_returns_every_image_of_short_and_long_plans():
    lib = _lib.load()
    counts = {}
    for name, (n, ops) in _lists().items():
        count = counts[name] = planner.pass_count(n, ops)
        images = planner.plan_ops(n, ops)
        assert images.dtype == planner.PASS_IMAGE and len(images) == count, name
        nq, qubits, mats = pack_ops(ops)
        direct = np.zeros(count + 8, dtype=planner.PASS_IMAGE)
        k = C.c_int32()
        _lib.check(lib.qsim_plan_ops(n, len(nq), _lib.ptr(nq), _lib.ptr(qubits), _lib.ptr(mats), _lib.ptr(direct), direct.nbytes, C.byref(k)))
        assert k.value == count and images.tobytes() == direct[:count].tobytes(), name
    assert 2 <= counts["short"] <= 64 < counts["long"], counts


def test_searched_tiles_are_the_tiles_of_the_plan_that_names_them():
    n, ops = _lists()["short"]
    masks = planner.search_tiles(n, ops)
    assert masks.dtype == np.uint64 and 2 <= len(masks) <= planner.pass_count(n, ops)
    images = planner.plan_ops(n, ops, tiles=masks)
    np.testing.assert_array_equal(planner.tile_masks(images), masks)
    assert [sum(1 << b for b in planner.tile_bits(img)) for img in images] == [int(m) for m in masks]


def test_peek_is_the_first_pass_of_the_plan():
    n, ops = _lists()["short"]
    done, members = np.zeros(len(ops), dtype=np.uint8), np.zeros(len(ops), dtype=np.int32)
    mask, need, held = planner.peek_pass(n, n, *pack_ops(ops), done, members)
    assert mask == int(planner.tile_masks(planner.plan_ops(n, ops))[0])
    assert need & ~mask == 0 and held == sorted(held) and 0 < len(held) <= len(ops)


def test_parallel_callers_get_what_one_caller_gets():
    """Eight threads, a different list each, 20 plans each: no buffer is shared between calls."""
    lists = [_rand_ops(12, 20, 100 + s) for s in range(8)]
    alone = [planner.plan_ops(12, ops).tobytes() for ops in lists]
    assert len(set(alone)) == len(alone)

    def work(i):
        return [planner.plan_ops(12, lists[i]).tobytes() for _ in range(20)]
    with ThreadPoolExecutor(8) as pool:
        for i, got in enumerate(pool.map(work, range(8))):
            assert all(g == alone[i] for g in got), i
