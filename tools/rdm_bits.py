"""The bits of the two reduced-density-matrix calls, to compare two builds of the library (QSIM_LIBRARY selects the
build):

    python tools/rdm_bits.py out.json

Per case the SHA-256 of the result matrix on an `init_random` state with a fixed seed, for three qubit lists: the low r
bits, the top r bits, and a fixed-seed shuffle that contains a line bit and the top bit (r = 1: bit 1).  r = 1..6
(`qsim_reduced_density_matrix`) at n = r, r + 1, 10, 11, 12 and 14 qubits -- chunks below a tile, one tile, the
grid-stride loop -- and r = 1, 3, 6 at 23 (four tiles per workgroup); r = 7..10 (`qsim_reduced_density_matrix_wide`) at
n = r, r + 1, r + 5 and 14, r = 7 at 23 and r = 8 at 22 (a workgroup walks four outer tiles), r = 11 and 12 at n = r and
14; r = 3, 6 and 7 on a 2^22 view at offset 5 * 2^22 inside a 2^25 parent (the streaming instantiation).  Two builds
that sum in the same order give equal files.
"""
from __future__ import annotations

import hashlib
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from quantum_simulations_amd.kernel.device import DeviceChunk  # noqa: E402


def sizes(r: int) -> list:
    if r <= 6:
        ns = [r, r + 1, 10, 11, 12, 14] + ([23] if r in (1, 3, 6) else [])
    elif r <= 10:
        ns = [r, r + 1, r + 5, 14] + ({7: [23], 8: [22]}.get(r, []))
    else:
        ns = [r, 14]
    return sorted({n for n in ns if n >= r})


def qubit_lists(n: int, r: int) -> dict:
    rng = np.random.default_rng(100 * n + r)
    if r == 1:
        mixed = [min(1, n - 1)]
    else:
        line, top = int(rng.integers(0, min(3, n - 1))), n - 1
        rest = [q for q in range(n) if q not in (line, top)]
        mixed = [line, top] + [int(q) for q in rng.permutation(rest)[: r - 2]]
        mixed = [mixed[i] for i in rng.permutation(r)]
    return {"low": list(range(r)), "top": list(range(n - r, n)), "mixed": mixed}


def matrices(c: DeviceChunk, n: int, r: int) -> dict:
    call = c.reduced_density_matrix if r <= 6 else c.reduced_density_matrix_wide
    return {name: {"qubits": qs, "sha256": hashlib.sha256(call(qs).tobytes()).hexdigest()}
            for name, qs in qubit_lists(n, r).items()}


def run() -> dict:
    out = {}
    by_size = {}
    for r in range(1, 13):
        for n in sizes(r):
            by_size.setdefault(n, []).append(r)
    for n in sorted(by_size):
        c = DeviceChunk.empty(n)
        try:
            c.init_random(1000 + n)
            for r in by_size[n]:
                out[f"r={r} n={n}"] = matrices(c, n, r)
        finally:
            c.close()
    parent = DeviceChunk.empty(25)
    view = parent.view(5 << 22, 22)
    try:
        parent.init_random(25)
        for r in (3, 6, 7):
            out[f"r={r} n=22 view in 25"] = matrices(view, 22, r)
    finally:
        view.close()
        parent.close()
    return out


if __name__ == "__main__":
    res = run()
    Path(sys.argv[1]).parent.mkdir(parents=True, exist_ok=True)
    Path(sys.argv[1]).write_text(json.dumps(res, indent=1, sort_keys=True) + "\n")
    print(json.dumps({"tool": "tools/rdm_bits.py", "cases": len(res), "sha256": hashlib.sha256(json.dumps(res, sort_keys=True).encode()).hexdigest()}))
