#!/usr/bin/env python3
"""Generate pauli_plans.json: the pass plans of qsim_plan_expectation and qsim_plan_pauli_rotations, recorded from a build
of the library that is known good (select it with QSIM_LIBRARY; the fixture in the tree comes from the commit before
the two planners were folded into one).

    QSIM_LIBRARY=/path/to/known-good/libqsim_hip.so python tests/golden/make_pauli_plans.py

Seeded random lists of X masks for k = 0 .. 30 index bits -- short ones, lists of x = 0 only, lists with wide terms
(x on more bits than a tile holds), a few longer than the 1024 terms of a pass -- and the Heisenberg chain at 30.
tests/test_pauli_plans_golden.py asserts that the library in the tree plans every list the same way."""
from __future__ import annotations

import json
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))

from quantum_simulations_amd.kernel import planner  # noqa: E402
from quantum_simulations_amd.kernel.device import plan_expectation  # noqa: E402


def mask(rng, k: int, weight: int) -> int:
    return int(sum(1 << int(b) for b in rng.choice(k, size=min(weight, k), replace=False))) if k else 0


def lists():
    rng = np.random.default_rng(20)
    yield 5, []
    for k in range(31):
        for rep in range(8):                                  # short lists: weights 0..4, now and then a wide term
            n = int(rng.integers(1, 13))
            yield k, [mask(rng, k, 14 if k >= 16 and rng.random() < 0.15 else int(rng.integers(0, 5))) for _ in range(n)]
        yield k, [0] * int(rng.integers(1, 6))                # x = 0 only
        yield k, [mask(rng, k, 12) for _ in range(3)]         # wide wherever k holds 12 bits
    for k in (2, 11, 13, 30):                                 # passes split at 1024 terms
        yield k, [0] * 1030
        yield k, [mask(rng, k, int(rng.integers(0, 3))) for _ in range(1100)]
    inside = [0, 1, 2, 4, 5, 7, 8, 9, 10, 11, 12]             # one 11-bit tile, a wide term in the middle, Z-only strings
    long = [int(sum(1 << inside[int(b)] for b in rng.choice(11, size=int(rng.integers(0, 4)), replace=False))) for _ in range(1300)]
    long[500] = (1 << 26) - 1
    yield 30, long
    heis = []
    for a in range(29):
        heis += [3 << a, 3 << a, 0]                           # XX, YY, ZZ
    yield 30, heis


def main() -> None:
    cases = []
    for k, x in lists():
        xs = np.array(x, dtype=np.uint64)
        e_pass, e_tiles = plan_expectation(k, xs)
        r_pass, r_tiles = planner.plan_pauli_rotations(k, xs)
        cases.append({"k": k, "x": [int(v) for v in x],
                      "expectation": {"pass_of": [int(v) for v in e_pass], "tiles": [int(v) for v in e_tiles]},
                      "rotations": {"pass_of": [int(v) for v in r_pass], "tiles": [int(v) for v in r_tiles]}})
    with open(HERE / "pauli_plans.json", "w") as f:
        json.dump(cases, f, separators=(",", ":"))
    print(len(cases), "lists,", (HERE / "pauli_plans.json").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
