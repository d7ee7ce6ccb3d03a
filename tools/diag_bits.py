"""The bits of the five diagonal calls, to compare two builds of the library (QSIM_LIBRARY selects the build):

    python tools/diag_bits.py out.json

Per size (1, 5, 10, 11, 12, 14, 22 and 25 qubits: chunks below a tile, one tile, the grid-stride loop, the streaming
instantiations) on `init_random` states with fixed seeds, and per term list (empty; one term; 40 terms of one in-tile
mask, so pieces and a join run; 2049 random masks, two passes of the per-term call): the outputs of
`qsim_diagonal_moments`, `qsim_overlap_diagonal` and `qsim_expectation_z_terms` as hex floats, and for the phase and the
sum written, accumulated and in place the SHA-256 of the downloaded state (up to 14 qubits) or its fingerprint (above).
Two builds that sum in the same order give equal files.
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

SIZES = (1, 5, 10, 11, 12, 14, 22, 25)
TILE_BITS = 11


def term_lists(n: int) -> dict:
    rng = np.random.default_rng(1000 + n)
    inner = (1 << min(n, TILE_BITS)) - 1
    same = (rng.integers(0, 1 << n, size=40, dtype=np.uint64) & np.uint64(~inner & ((1 << n) - 1))) | np.uint64(5 & inner)
    lists = {"empty": np.zeros(0, dtype=np.uint64), "one": np.array([(1 << n) - 1], dtype=np.uint64), "same_inner_40": same,
             "random_2049": rng.integers(0, 1 << n, size=2049, dtype=np.uint64)}
    return {name: (z, rng.standard_normal(z.size) / max(z.size, 1)) for name, z in lists.items()}


def state_bits(c: DeviceChunk, n: int) -> str:
    if n <= 14:
        return hashlib.sha256(c.download().tobytes()).hexdigest()
    f = c.fingerprint(n, seed=7)
    return f"{f.real.hex()} {f.imag.hex()}"


def run(n: int) -> dict:
    psi, phi, work = (DeviceChunk.empty(n) for _ in range(3))
    res = {}
    try:
        psi.init_random(1)
        phi.init_random(2)
        for name, (z, co) in term_lists(n).items():
            values = psi.expectation_z_terms(z)
            row = {"moments": [v.hex() for v in psi.diagonal_moments(z, co)],
                   "overlap": [v.hex() for q in psi.overlap_diagonal(phi, z, co) for v in (q.real, q.imag)],
                   "z_terms": hashlib.sha256(values.tobytes()).hexdigest(), "z_terms_head": [float(v).hex() for v in values[:4]]}
            work.copy_from(psi)
            work.apply_diagonal_phase(z, co, 0.37)
            row["phase"] = state_bits(work, n)
            work.apply_diagonal_sum(psi, z, co)
            row["sum_written"] = state_bits(work, n)
            work.apply_diagonal_sum(phi, z, co, accumulate=True)
            row["sum_accumulated"] = state_bits(work, n)
            work.apply_diagonal_sum(work, z, co)
            row["sum_in_place"] = state_bits(work, n)
            res[name] = row
    finally:
        for c in (psi, phi, work):
            c.close()
    return res


if __name__ == "__main__":
    out = {str(n): run(n) for n in SIZES}
    Path(sys.argv[1]).parent.mkdir(parents=True, exist_ok=True)
    Path(sys.argv[1]).write_text(json.dumps(out, indent=1, sort_keys=True) + "\n")
    print(json.dumps({"tool": "tools/diag_bits.py", "sizes": list(SIZES), "sha256": hashlib.sha256(json.dumps(out, sort_keys=True).encode()).hexdigest()}))
