"""DistributedEngine.expectation with the real HIP shard backend: 2 and 4 ranks share cuda:0 (exchange over gloo, the
rehearsal set-up of test_gpu_distributed.py), a circuit runs, then a Pauli sum whose X/Y terms touch rank bits is
evaluated and checked against the one-GPU SingleGpuEngine.expectation of the same circuit at 1e-12."""
import os
import sys
import traceback
from pathlib import Path

import numpy as np
import pytest
import torch.multiprocessing as mp

from tests.test_distributed_gloo import _free_port
from tests.test_expectation_gloo import _observable

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def _circuit(n):
    from quantum_simulations_amd import circuits as gen
    return gen.random_1q_cx_circuit(n, depth=8, seed=13)


def _worker(rank, world, port, n, out, errors):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
        sys.path.insert(0, str(ROOT))
        from quantum_simulations_amd.runner.distributed import DistributedEngine, HipShardBackend
        p = world.bit_length() - 1
        obs = _observable(n)
        for staging in (True, False):
            eng = DistributedEngine(n, world, rank, backend=HipShardBackend(n - p, 0), staging=staging,
                                    relayout_pieces=2, min_piece_qubits=1)
            eng.init_zero_state()
            plan = eng.plan(_circuit(n), repeats=2)
            eng.execute(plan)
            before = eng.state_vector()
            got = eng.expectation(obs)
            assert np.array_equal(eng.state_vector(), before)
            eng.execute(plan)                          # the plan still runs after the moves of the expectation
            got2 = eng.expectation(obs)
            out.put((rank, staging, got.hex(), got2.hex()))
            eng.backend.close()
        eng.close()
    except Exception:
        errors.put((rank, traceback.format_exc()))
        raise


@pytest.mark.parametrize("world,n", [(2, 12), (4, 14)])
def test_ranks_sharing_one_gpu(world, n):
    from quantum_simulations_amd.runner.engine import SingleGpuEngine
    ctx = mp.get_context("spawn")
    errors, out = ctx.SimpleQueue(), ctx.SimpleQueue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, n, out, errors)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(300)
    msgs = []
    while not errors.empty():
        msgs.append(errors.get())
    for p in procs:
        if p.is_alive():
            p.kill()
            p.join(10)
            msgs.append((-1, "worker still running after 300 s: killed"))
    assert not msgs and all(p.exitcode == 0 for p in procs), "\n".join(f"[rank {r}] {m}" for r, m in msgs)
    rows = []
    while not out.empty():
        rows.append(out.get())
    assert len(rows) == 2 * world
    eng = SingleGpuEngine(n, layout="identity")
    try:
        obs = _observable(n)
        eng.init_zero_state()
        plan = eng.plan(_circuit(n))
        eng.execute(plan)
        want = eng.expectation(obs)
        eng.execute(plan)
        want2 = eng.expectation(obs)
    finally:
        eng.close()
    for staging in (True, False):
        vals = {(r[2], r[3]) for r in rows if r[1] == staging}
        assert len(vals) == 1, vals                   # every rank: identical bits
        got, got2 = (float.fromhex(v) for v in vals.pop())
        assert abs(got - want) < 1e-12 and abs(got2 - want2) < 1e-12, (staging, got - want, got2 - want2)
