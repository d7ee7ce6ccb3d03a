"""The measured price of the fused pass's gate engine (round 19).

A fused pass costs max(memory time of its tile, engine time of its records).  The memory side is the tile-cost model of
`runner/tile_layout.py`; this module holds the engine side: microseconds per record kind, fitted to a few hundred one-pass
op lists timed on MI355X (`tools/engine_cost_sample.py` -> `tools/fit_engine_cost_model.py`; the numbers ship as
`engine_cost_model.json`).  The library reads nothing itself: `table()` is handed to its priced planning calls
(`planner.rewrite_ops`, `planner.balance`) as an argument, in the order of the QSIM_ENGINE_COST_* entries of
include/qsim_hip.h; `None` instead of a table switches the pricing off.
"""
from __future__ import annotations

import json
from pathlib import Path

import numpy as np

_MODEL_PATH = Path(__file__).resolve().parent / "engine_cost_model.json"
# QSIM_ENGINE_COST_* (include/qsim_hip.h), in order
ENTRIES = ("fixed_us", "group", "dense1", "real1", "had1", "swap1", "aswap1", "anti1", "phase", "phase_neg", "phase_i", "diagr",
           "dense2", "pred_lane", "pred_outer", "reg_ctrl", "direct_end", "fit_qubits", "unit1")
_table: np.ndarray | None = None


def table() -> np.ndarray:
    """The shipped cost table as the float64 array the library's priced calls take."""
    global _table
    if _table is None:
        costs = json.loads(_MODEL_PATH.read_text())["costs_us"]
        _table = np.array([float(costs[name]) for name in ENTRIES], dtype=np.float64)
    return _table
