"""One `name sha256` line per case of a fixed corpus of op lists, over the bytes of what the host planner makes of it:
pass images, searched tiles, rewritten lists, layout counts, peeked passes.  Two builds of the library plan alike when
their outputs are equal (QSIM_LIBRARY names the build, as for the tests' child processes; knobs move the probe build).
Needs no device.  A tool for comparing builds: no hashes are kept, a better planner changes them."""
import hashlib
import itertools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import dense_oracle as orc  # noqa: E402
from quantum_simulations_amd import circuits  # noqa: E402
from quantum_simulations_amd.circuit.fusion import batch_levels  # noqa: E402
from quantum_simulations_amd.circuit.io import levelize, validate_circuit_dict  # noqa: E402
from quantum_simulations_amd.kernel import planner  # noqa: E402
from quantum_simulations_amd.kernel.device import pack_ops  # noqa: E402
from quantum_simulations_amd.runner.engine import gate_ops  # noqa: E402
from tests import engine_cases  # noqa: E402
from tests.test_gpu_kernels import _random_ops  # noqa: E402
from tests.test_tile_planner_cpu import _long_list_with_a_control_only_qubit  # noqa: E402


def show(name, *arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    print(name, h.hexdigest(), flush=True)


def rewritten(n, ops):
    out = planner.rewrite_ops(n, ops)
    return out, [np.array(q + [len(q)], dtype=np.int32) for q, _ in out] + [U for _, U in out]


def plan(name, n, ops, search=False):
    show(name + ".plan", planner.plan_ops(n, ops))
    if search:
        tiles = planner.search_tiles(n, ops)
        show(name + ".tiles", tiles)
        show(name + ".tiled", planner.plan_ops(n, ops, tiles))


def main():
    batches = batch_levels(levelize(validate_circuit_dict(circuits.random_1q_cx_circuit(28, depth=40))), 28)
    for n in (28, 30):
        for b, batch in enumerate(batches):
            ops, name = batch["local_ops"], f"bench{n}.{b}"
            plan(name, n, ops, search=True)
            rw, rw_bytes = rewritten(n, ops)
            show(name + ".rewrite", *rw_bytes)
            plan(name + ".rw", n, rw, search=True)
    for n in (13, 22, 33):
        plan(f"ghz_qft{n}", n, gate_ops(validate_circuit_dict(circuits.generate_ghz_qft(n))))
        plan(f"qft{n}", n, gate_ops(validate_circuit_dict(circuits.generate_qft_circuit(n))))
    for n in (12, 26):
        ops = gate_ops(validate_circuit_dict(circuits.random_clifford_t_circuit(n)))
        plan(f"clifford_t{n}", n, ops, search=n == 12)
        show(f"clifford_t{n}.rewrite", *rewritten(n, ops)[1])
    for n in range(8, 19):
        for seed in range(3):
            plan(f"random{n}.{seed}", n, _random_ops(n, 120, 1000 * n + seed), search=seed == 0)
    for c in engine_cases.directed_lists():
        plan("case." + engine_cases.case_id(c), c.n, c.ops)
    plan("control_only28", 28, _long_list_with_a_control_only_qubit(28, 4000, 1))
    plan("control_only13", 13, _long_list_with_a_control_only_qubit(13, 2500, 5))
    SW = orc.gate_matrix("SWAP", {})
    for n, m in itertools.product((9, 11, 12), (1, 2, 3)):
        for los in itertools.combinations(range(4), m):
            plan(f"staging{n}." + "".join(map(str, los)), n, [([lo, hi], SW) for lo, hi in zip(los, range(n - m, n))])
    # a peek walk: a 30-qubit list on 27 local bits, pass by pass until nothing local is left
    nq, qubits, mats = pack_ops(gate_ops(validate_circuit_dict(circuits.random_1q_cx_circuit(30, depth=12))))
    done, members = np.zeros(len(nq), dtype=np.uint8), np.zeros(len(nq), dtype=np.int32)
    for step in range(64):
        mask, need, mem = planner.peek_pass(27, 30, nq, qubits, mats, done, members, avoid=7 << 24)
        show(f"peek.{step}", np.array([mask, need], dtype=np.uint64), np.array(mem, dtype=np.int64))
        if not mem:
            break
        done[mem] = 1
    rng = np.random.default_rng(7)
    layouts = np.array([rng.permutation(28) for _ in range(16)], dtype=np.int32)
    show("count_layouts", planner.count_layouts(28, batches[0]["local_ops"], layouts, 4))


if __name__ == "__main__":
    main()
