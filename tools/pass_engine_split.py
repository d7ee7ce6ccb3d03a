#!/usr/bin/env python3
"""Engine / memory split of every pass of the TIMED bench plan: per pass its tile bits, records by kind, register
groups, HIP-event ms with its gates, and the gate-less ms (load -> LDS -> store) of the same tile in the same session.

    python3 tools/pass_engine_split.py [n_qubits] [depth]          the table (two child processes, one after the other)
    python3 tools/pass_engine_split.py --gated N DEPTH OUT.json    child 1: plan as bench.py does, time every pass
    python3 tools/pass_engine_split.py --gateless N OUT.json       child 2: the gate-less pass over each of those tiles

The knobs are read by the probe library when it loads, so each configuration is a process of its own; the parent never
opens the device.  The record kinds come from the pass images the host planner writes for the same ops and tiles
(no device involved), walked as the engine walks them."""
import json
import os
import re
import subprocess
import sys
from collections import Counter
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
os.environ.setdefault("QSIM_LIBRARY", str(ROOT / "quantum_simulations_amd" / "libqsim_hip_probes.so"))
sys.path.insert(0, str(ROOT))

_TIMED = re.compile(r"\[qsim\] timed pass: ([0-9.]+) ms, (\d+) records, high bits((?: \d+)+)")


def record_kinds(n, ops, tiles):
    """per pass: (Counter of record kinds, register groups) from the planner's pass images"""
    from quantum_simulations_amd.kernel import planner
    from tests import tile_interpreter as ti
    out = []
    for img in planner.plan_ops(n, ops, tiles):
        kinds, groups = Counter(), 0
        for rec in ti.records(img):
            if rec[0] == "group":
                groups += 1
                continue
            _, case, blk, outer = rec[:4]
            name = ti.fam_of(case)
            if name in ("DENSE1", "REAL1", "HAD1", "SWAP1", "ANTI1", "YLIKE1", "ASWAP1") and case - ti.OPC[name] >= 3:
                name += "c"                                   # controlled from a register bit
            if blk:
                name += "+lane"
            if outer:
                name += "+outer"
            kinds[name] += 1
        # ends of the pass that move between global memory and registers directly (no LDS trip): not records, priced per end
        kinds["direct_ends"] = bin(int(img["order"]) & (ti.DIRECT_IN | ti.DIRECT_OUT)).count("1")
        out.append((dict(kinds), groups))
    return out


def child_gated(n, depth, out_path):
    os.environ["QSIM_DEBUG_STATS"] = "2"
    from quantum_simulations_amd.circuits import random_1q_cx_circuit
    from quantum_simulations_amd.runner.engine import make_engine
    eng = make_engine(n, layout="search", tune_on_device=True)
    eng.init_zero_state()
    plan = eng.plan(random_1q_cx_circuit(n, depth=depth), repeats=25)
    eng.execute(plan)
    eng.barrier()
    print("---- timed executions ----", file=sys.stderr, flush=True)
    for _ in range(3):
        eng.execute(plan)
        eng.barrier()
    norm2 = eng.norm2()
    eng.close()
    kinds = []
    for packed, masks in zip(plan, plan.tiles):
        kinds += record_kinds(n, packed, masks)
    info = {k: v for k, v in getattr(plan, "layout_info", {}).items() if k in ("model_ms", "passes_chosen", "seconds")}
    json.dump({"n": n, "depth": depth, "norm2": norm2, "info": info,
               "kinds": [k for k, _ in kinds], "groups": [g for _, g in kinds]}, open(out_path, "w"))


def child_gateless(n, out_path):
    os.environ["QSIM_DEBUG_SKIP_GATES"] = "4"
    tiles = json.load(open(out_path))["tiles"]
    os.environ["QSIM_DEBUG_TILE_BITS"] = ",".join(str(b) for b in tiles[0])
    import numpy as np
    from quantum_simulations_amd.kernel import gates as gt
    from quantum_simulations_amd.kernel.device import DeviceChunk
    dev = DeviceChunk.empty(n)
    dev.init_random(1)
    ops = [([3], gt.H()), ([4], gt.H())]
    ms = []
    for bits in tiles:
        os.environ["QSIM_DEBUG_TILE_BITS"] = ",".join(str(b) for b in bits)
        dev.apply_ops(ops)
        dev.sync()
        ts = []
        for _ in range(7):
            dev.time_begin()
            dev.apply_ops(ops)
            ts.append(dev.time_end())
        ms.append(float(np.median(ts)))
    doc = json.load(open(out_path))
    doc["gateless_ms"] = ms
    json.dump(doc, open(out_path, "w"))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--gated":
        return child_gated(int(sys.argv[2]), int(sys.argv[3]), sys.argv[4])
    if len(sys.argv) > 1 and sys.argv[1] == "--gateless":
        return child_gateless(int(sys.argv[2]), sys.argv[3])
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 28
    depth = int(sys.argv[2]) if len(sys.argv) > 2 else 40
    tmp = ROOT / "profile_out"
    tmp.mkdir(exist_ok=True)
    path = str(tmp / f"pass_engine_split_{n}.json")
    a = subprocess.run([sys.executable, __file__, "--gated", str(n), str(depth), path], stderr=subprocess.PIPE, text=True, timeout=400)
    if a.returncode:
        sys.stderr.write(a.stderr[-4000:])
        sys.exit(a.returncode)
    timed = a.stderr.split("---- timed executions ----")[1]
    rows = [(float(m.group(1)), int(m.group(2)), [int(b) for b in m.group(3).split()]) for m in _TIMED.finditer(timed)]
    doc = json.load(open(path))
    n_pass = len(doc["kinds"])
    assert len(rows) == 3 * n_pass, (len(rows), n_pass)
    doc["tiles"] = [r[2] for r in rows[:n_pass]]
    json.dump(doc, open(path, "w"))
    b = subprocess.run([sys.executable, __file__, "--gateless", str(n), path], timeout=200)
    if b.returncode:
        sys.exit(b.returncode)
    doc = json.load(open(path))
    print(f"# {n} qubits, depth {depth}: the timed plan, {n_pass} passes; model_ms {doc['info'].get('model_ms')}; norm2 {doc['norm2']:.12f}")
    print("# pass  records groups  gated_ms  gateless_ms  diff_ms  tile bits / records by kind")
    tot_g = tot_0 = 0.0
    doc["gated_ms"] = [sorted(rows[p + r * n_pass][0] for r in range(3))[1] for p in range(n_pass)]
    json.dump(doc, open(path, "w"))
    for p in range(n_pass):
        gated = doc["gated_ms"][p]
        nrec = rows[p][1]
        free = doc["gateless_ms"][p]
        tot_g += gated
        tot_0 += free
        kinds = " ".join(f"{k}={v}" for k, v in sorted(doc["kinds"][p].items()))
        print(f"{p:4d}  {nrec:7d} {doc['groups'][p]:6d}  {gated:8.3f}  {free:11.3f}  {gated - free:7.3f}  {','.join(map(str, rows[p][2]))} | {kinds}")
    print(f"# sum   gated {tot_g:.3f} ms   gate-less {tot_0:.3f} ms   gated - gate-less {tot_g - tot_0:.3f} ms = {100 * (tot_g - tot_0) / tot_g:.1f} % of the step")


if __name__ == "__main__":
    main()
