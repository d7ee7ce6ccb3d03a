#!/usr/bin/env python3
"""Fit the engine cost table (runner/engine_cost_model.json) to the samples of tools/engine_cost_sample.py.

    python3 tools/fit_engine_cost_model.py samples.json gateless_ms [out.json [pass_engine_split.json ...]]

Model of a pass: ms = max(memory ms of its tile, fixed + sum over its records of the kind's cost + groups * group cost
+ direct ends * what an end that moves between global memory and registers without its LDS trip saves).
`gateless_ms` is the measured gate-less time of the sampled tile.  Only passes that are clearly engine bound (measured
above the gate-less time by more than `MARGIN`) enter the least-squares fit; costs are kept non-negative except the
predicated forms: a record under a predicate on tile bits outside the register group (lane), on index bits outside
the tile (outer) or with its control on a register bit costs a FRACTION of the plain record (only the amplitudes, waves or
tiles the predicate selects do the work); the three fractions are searched on a grid.  Kinds the samples do not hold are priced from
their neighbours by the instruction counts of csrc/tile_ops.h (anti-diagonal 40 : real 32, dense 4x4 144 : dense 2x2 68).
Prints the table, the residuals of the fit and of the held-out third.

Calibration (optional, the documents tools/pass_engine_split.py leaves): on the engine-bound passes of the timed bench
plans the fitted model ran uniformly high (measured / modelled 0.90 +- 0.02 at 28 qubits: random lists on few targets are
dearer than a circuit's passes); every cost is scaled by the mean ratio of those passes, which is recorded."""
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
FAMILIES = ["DENSE1", "REAL1", "HAD1", "SWAP1", "ASWAP1", "PHASE", "PHASE_NEG", "PHASE_I", "DIAGR"]
MARGIN = 0.10          # ms above the gate-less pass from which a sample counts as engine bound


def features(row, factor):
    """record counts per family, a predicated record counted as the fraction `factor` of a plain one"""
    f = dict.fromkeys(FAMILIES, 0.0)
    for name, count in row["kinds"].items():
        if name == "direct_ends":
            continue
        parts = name.split("+")
        fam, w = parts[0], float(count)
        if fam.endswith("c") and fam[:-1] in ("DENSE1", "REAL1", "HAD1", "SWAP1", "ASWAP1", "ANTI1", "YLIKE1"):
            fam = fam[:-1]
            w *= factor["regctrl"]
        fam = {"PHASE_NI": "PHASE_I", "SCALE": "PHASE", "ANTI1": "REAL1", "YLIKE1": "REAL1"}.get(fam, fam)
        for p in parts[1:]:
            w *= factor[p]
        f[fam] += w
    return [f[k] for k in FAMILIES] + [float(row["groups"]), 1.0, float(row["kinds"].get("direct_ends", 0))]


def solve(X, y):
    """least squares with the costs kept non-negative (a negative one is pinned to zero, the worst first)"""
    coef = np.zeros(X.shape[1])
    active = np.ones(X.shape[1], dtype=bool)
    for _ in range(X.shape[1]):
        coef[:] = 0
        coef[active] = np.linalg.lstsq(X[:, active], y, rcond=None)[0]
        neg = [i for i in np.flatnonzero(active) if coef[i] < 0 and i != X.shape[1] - 1]      # (a direct end SAVES an LDS trip)
        if not neg:
            break
        active[min(neg, key=lambda i: coef[i])] = False
    return coef, float(np.sum((X @ coef - y) ** 2))


def main():
    doc = json.load(open(sys.argv[1]))
    mem = float(sys.argv[2])
    out = sys.argv[3] if len(sys.argv) > 3 else str(ROOT / "quantum_simulations_amd" / "runner" / "engine_cost_model.json")
    rows = doc["rows"]
    y = np.array([r["ms"] for r in rows]) * 1e3                       # microseconds
    held = np.arange(len(rows)) % 3 == 2
    use = (y > (mem + MARGIN) * 1e3) & ~held
    names = FAMILIES + ["group", "fixed", "direct_end"]
    # the three factors of the predicated forms are searched on a grid, the costs solved linearly inside
    grid = [round(0.3 + 0.05 * i, 2) for i in range(15)]
    best = None
    for fl in grid:
        for fo in grid:
            for fr in grid:
                factor = {"lane": fl, "outer": fo, "regctrl": fr}
                X = np.array([features(r, factor) for r in rows])
                coef, sse = solve(X[use], y[use])
                if best is None or sse < best[0]:
                    best = (sse, factor, coef, X)
    _, factor, coef, X = best
    pred = np.maximum(mem * 1e3, X @ coef)

    def err(mask):
        e = (pred[mask] - y[mask]) / y[mask]
        return float(np.sqrt(np.mean(e ** 2))), float(np.max(np.abs(e)))
    c = dict(zip(names, (float(round(v, 2)) for v in coef)))
    table = {"fit_qubits": doc["n"], "fixed_us": c["fixed"], "group": c["group"], "dense1": c["DENSE1"], "real1": c["REAL1"],
             "had1": c["HAD1"], "swap1": c["SWAP1"], "aswap1": c["ASWAP1"], "anti1": round(c["REAL1"] * 40 / 32, 2),
             "phase": c["PHASE"], "phase_neg": c["PHASE_NEG"], "phase_i": c["PHASE_I"], "diagr": c["DIAGR"],
             "dense2": round(c["DENSE1"] * 144 / 68, 2), "pred_lane": factor["lane"], "pred_outer": factor["outer"],
             "reg_ctrl": factor["regctrl"], "direct_end": c["direct_end"],
             # (the samples count records in planned images, where a unit-diagonal real 2x2 is still REAL1: its price is
             # REAL1's times the ratio of the two one-pass slopes, measured with the lowering on and off: 0.75 - 0.78)
             # TODO: fit it as a family of its own (sample with the lowering off for REAL1 and on for UNIT1); 0.75 is the
             # lower end of profiles/r26a_ab_unit_real.txt section 1 (tools/gate_cost_probe.py, lowering on / off)
             "unit1": round(c["REAL1"] * 0.75, 2)}
    calibration = None
    ratios = []
    for path in sys.argv[4:]:
        split = json.load(open(path))
        scale = 2.0 ** (split["n"] - doc["n"])
        for p, (kinds, groups, free) in enumerate(zip(split["kinds"], split["groups"], split["gateless_ms"])):
            gated = split["gated_ms"][p]
            if gated > free + MARGIN * scale:
                model = float(np.dot(features({"kinds": kinds, "groups": groups}, factor), coef)) * scale / 1e3
                ratios.append(gated / model)
    if ratios:
        k = float(np.mean(ratios))
        calibration = {"scale": round(k, 4), "passes": len(ratios), "spread": round(float(np.std(ratios)), 4)}
        for key in table:
            if key not in ("fit_qubits", "pred_lane", "pred_outer", "reg_ctrl"):
                table[key] = round(table[key] * k, 2)
    rms_fit, max_fit = err(use)
    rms_held, max_held = err(held)
    rms_all, max_all = err(np.ones(len(rows), dtype=bool))
    doc_out = {"what": "microseconds one record of each kind adds to a fused pass of 2^fit_qubits amplitudes on MI355X; a pass costs "
                       "max(memory time of its tile, fixed_us + group * register groups + direct_end * ends without an LDS trip + its records); pred_lane / pred_outer / reg_ctrl are the "
                       "fractions of its plain cost that a predicated record costs",
               "fitted_by": "tools/fit_engine_cost_model.py <- tools/engine_cost_sample.py",
               "samples": {"passes": len(rows), "engine_bound_in_fit": int(use.sum()), "tile": doc["tile"], "gateless_ms": mem,
                           "rms_rel_error_fit": round(rms_fit, 4), "rms_rel_error_held_out": round(rms_held, 4),
                           "max_rel_error_held_out": round(max_held, 4), "rms_rel_error_all": round(rms_all, 4)},
               "calibration_on_bench_passes": calibration, "costs_us": table}
    Path(out).write_text(json.dumps(doc_out, indent=1) + "\n")
    for k, v in table.items():
        print(f"{k:12s} {v:9.2f}")
    print(f"fit on {int(use.sum())} engine-bound passes: rms {100 * rms_fit:.1f} %, max {100 * max_fit:.1f} %; held out ({int(held.sum())}): "
          f"rms {100 * rms_held:.1f} %, max {100 * max_held:.1f} %; all {len(rows)}: rms {100 * rms_all:.1f} %, max {100 * max_all:.1f} %")


if __name__ == "__main__":
    main()
