"""DistributedEngine.expectation on CPU: world 2 / 4 / 8 `gloo` process groups over a numpy shard double whose
`expectation_pauli` restates the device formula.  Terms with X/Y and Z on rank bits, checked against the one-state
numpy value; every rank returns the same bits; afterwards the logical state is unchanged and a following `execute`
is still correct."""
import os
import sys
import traceback
from pathlib import Path

import numpy as np
import pytest
import torch.multiprocessing as mp

from tests.test_distributed_gloo import _free_port

ROOT = Path(__file__).resolve().parent.parent


def _observable(n):
    from quantum_simulations_amd.observable import PauliSum
    rng = np.random.default_rng(11)
    terms = [(0.7, {n - 1: "Z"}), (-0.3, {n - 1: "X"}), (0.45, {n - 2: "Y", n - 1: "Y"}), (1.1, {0: "X", n - 1: "Y"}),
             (0.2, {0: "Z", 1: "Z"}), (-0.8, {1: "Y", n - 3: "X", n - 1: "Z"}), (0.5, {}), (0.9, {n - 2: "Z", n - 1: "X"})]
    for _ in range(24):
        qs = rng.choice(n, size=int(rng.integers(1, 5)), replace=False)
        terms.append((float(rng.standard_normal()), {int(q): "XYZ"[int(rng.integers(3))] for q in qs}))
    return PauliSum(terms, n_qubits=n)


def _worker(rank, world, port, n, out, errors):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
        sys.path.insert(0, str(ROOT))
        from oracle import dense_oracle as orc
        from quantum_simulations_amd import circuits as gen
        from quantum_simulations_amd.circuit.io import validate_circuit_dict
        from quantum_simulations_amd.observable import pauli_terms_np
        from quantum_simulations_amd.runner.distributed import DistributedEngine
        from tests.cpu_shard_backend import CpuShardBackend

        class ExpectationShardBackend(CpuShardBackend):
            def expectation_pauli(self, x_masks, z_masks):
                return pauli_terms_np(self._c("state"), x_masks, z_masks)

        p = world.bit_length() - 1
        obs = _observable(n)
        cd = gen.random_1q_cx_circuit(n, depth=6, seed=21)
        vcd = validate_circuit_dict(cd)
        for staging, fuse in ((True, True), (False, True), (False, False)):
            eng = DistributedEngine(n, world, rank, backend=ExpectationShardBackend(n - p), staging=staging,
                                    fuse_relayout=fuse, relayout_pieces=2, min_piece_qubits=1)
            eng.init_zero_state()
            plan = eng.plan(cd, repeats=2)
            eng.execute(plan)
            want_psi = orc.simulate(vcd)
            want = obs.value(pauli_terms_np(want_psi, *obs.masks()))
            before = eng.state_vector()
            got = eng.expectation(obs)
            assert abs(got - want) < 1e-12, (staging, fuse, got, want)
            assert abs(eng.expectation(obs) - want) < 1e-12          # again, from the layout the first call left
            assert np.array_equal(eng.state_vector(), before)        # the logical state is unchanged
            eng.execute(plan)                                        # ... and the plan still runs on it
            want2 = want_psi.copy()
            for g in vcd["gates"]:
                U = orc.gate_matrix(g["gate"], g["params"])
                (orc.apply_1q if len(g["qubits"]) == 1 else orc.apply_2q)(want2, *g["qubits"], U)
            assert float(np.max(np.abs(eng.state_vector() - want2))) < 1e-12
            got2 = eng.expectation(obs)
            assert abs(got2 - obs.value(pauli_terms_np(want2, *obs.masks()))) < 1e-12
            out.put((rank, staging, fuse, got.hex(), got2.hex()))
            if p:
                wide = {q: "X" for q in range(n - p + 1)}            # X/Y on more qubits than a shard holds
                with pytest.raises(ValueError):
                    eng.expectation([(1.0, wide)])
            eng.backend.close()
            eng.close()
    except Exception:
        errors.put((rank, traceback.format_exc()))
        raise


@pytest.mark.parametrize("world,n", [(2, 8), (4, 8), (8, 8)])
def test_expectation_over_ranks(world, n):
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
            msgs.append((-1, "worker still running after 300 s (hung collective?): killed"))
    assert not msgs and all(p.exitcode == 0 for p in procs), "\n".join(f"[rank {r}] {m}" for r, m in msgs)
    rows = []
    while not out.empty():
        rows.append(out.get())
    assert len(rows) == 3 * world
    for mode in {(r[1], r[2]) for r in rows}:
        vals = {(r[3], r[4]) for r in rows if (r[1], r[2]) == mode}
        assert len(vals) == 1, (mode, vals)                          # every rank: identical bits
