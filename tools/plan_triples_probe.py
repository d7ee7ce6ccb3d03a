"""Host cost of the line-qubit triple search (`planner.search_triples`, qsim_plan_search_triples) on the rewritten bench
lists: seconds and the pass-count histogram for the engine's candidate list (identity + N random triples, the seed of
`choose_plan_layout`), with and without the shared bound, and with the bound that also counts needed tile bits, for
several thread counts.  No device.

    python tools/plan_triples_probe.py [--qubits 28 30] [--candidates 255] [--threads 1 8 16] [--all]

--all: every C(n, 3) triple instead (minutes), bounded, at the largest thread count only."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from quantum_simulations_amd.circuit.fusion import batch_levels  # noqa: E402
from quantum_simulations_amd.circuit.io import levelize, validate_circuit_dict  # noqa: E402
from quantum_simulations_amd.circuits import random_1q_cx_circuit  # noqa: E402
from quantum_simulations_amd.kernel import planner  # noqa: E402
from quantum_simulations_amd.runner.layout_search import candidate_triples  # noqa: E402

SEED = 20260504                    # choose_plan_layout's default


def bench_ops(n: int) -> list:
    batches = [p["local_ops"] for p in batch_levels(levelize(validate_circuit_dict(random_1q_cx_circuit(n, depth=40))), n)]
    assert len(batches) == 1
    return planner.rewrite_ops(n, batches[0])


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--qubits", type=int, nargs="+", default=[28, 30])
    ap.add_argument("--candidates", type=int, default=255)
    ap.add_argument("--threads", type=int, nargs="+", default=[1, 8, 16])
    ap.add_argument("--all", action="store_true")
    args = ap.parse_args()
    print(f"host threads available: {len(os.sched_getaffinity(0))}")
    for n in args.qubits:
        ops = bench_ops(n)
        triples = None if args.all else candidate_triples(n, args.candidates, SEED)
        print(f"n = {n}: {len(ops)} ops after the rewrite, {'all' if args.all else len(triples)} triples, default beam")
        modes = [("bounded", 0)] if args.all else [("unbounded", planner.TRIPLES_UNBOUNDED), ("bounded", 0),
                                                   ("bounded + need bits", planner.TRIPLES_NEED_BITS)]
        for threads in ([max(args.threads)] if args.all else args.threads):
            for name, flags in modes:
                t0 = time.perf_counter()
                res = planner.search_triples(n, ops, triples, 0, threads, flags)
                dt = time.perf_counter() - t0
                hist = ", ".join(f"{'more' if p is None else p}: {c}" for p, c in res["histogram"].items())
                print(f"  {threads:2d} threads  {name:20s} {dt:8.2f} s   fewest {res['passes']} on {len(res['index'])} of "
                      f"{res['searched']}   histogram {{{hist}}}", flush=True)


if __name__ == "__main__":
    main()
