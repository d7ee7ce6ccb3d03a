"""Dynamic circuits on one MI355X: where the time of a measurement round goes.

    python tools/dynamic_probe.py [out.json]

* qsim_probabilities at 30 qubits, r = 8 on mixed bits (bit 0 included) and on other bit sets, against qsim_norm2 on the
  same chunk, interleaved (median of 7): the histogram's read rate relative to the plain reduction;
* run_dynamic on a bwt-style program (x / cx / ccx, ancillas reset every 12 gates) and a square_root-style program (runs
  of 8 resets) at 28 and 30 qubits, and on QASMBench's square_root_n30 (tests/golden/qasmbench_cluster.tar.xz):
  rounds, fused passes, histogram time and rate, the histograms' share of device time, and host time per round
  (wall time minus the event time of every launch, divided by the launches a round costs).
The histograms' share of device time decides whether the histogram should later be folded into the store phase of the
fused pass before it.
"""
from __future__ import annotations

import json
import statistics
import sys
import tarfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from quantum_simulations_amd.circuit.dynamic import validate_dynamic  # noqa: E402
from quantum_simulations_amd.circuit.import_qasm import qasm_to_dynamic  # noqa: E402
from quantum_simulations_amd.circuits import dynamic_bwt_style_qasm, dynamic_square_root_style_qasm  # noqa: E402
from quantum_simulations_amd.kernel.device import DeviceChunk  # noqa: E402
from quantum_simulations_amd.runner.dynamic import run_dynamic  # noqa: E402


def rate_vs_norm2(n: int = 30, reps: int = 7) -> list[dict]:
    c = DeviceChunk.zero_state(n)
    out = []
    try:
        c.init_random(1)
        nbytes = 16.0 * (1 << n)
        sets = {"mixed r=8 incl. bit 0": [0, 4, 9, 13, 18, 22, 26, 29], "low r=8 (bits 0..7)": list(range(8)),
                "high r=8 (bits 22..29)": list(range(22, 30)), "unsorted r=3": [17, 1, 28], "r=1 bit 0": [0]}
        for name, qs in sets.items():
            t_h, t_n = [], []
            c.probabilities(qs)
            c.norm2()
            for _ in range(reps):
                c.time_begin()
                c.probabilities(qs)
                t_h.append(c.time_end())
                c.time_begin()
                c.norm2()
                t_n.append(c.time_end())
            mh, mn = statistics.median(t_h), statistics.median(t_n)
            out.append({"qubits": qs, "set": name, "hist_ms": mh, "norm2_ms": mn, "hist_GBps": nbytes / mh / 1e6,
                        "norm2_GBps": nbytes / mn / 1e6, "rate_ratio": mn / mh})
            print(json.dumps(out[-1]), flush=True)
    finally:
        c.close()
    return out


def run_one(label: str, prog: dict, seed: int = 1) -> dict:
    n = prog["number_of_qubits"]
    t0 = time.perf_counter()
    res = run_dynamic(prog, seed)
    wall = (time.perf_counter() - t0) * 1e3
    try:
        res.state.sync()
    finally:
        res.state.close()
    launches = res.histogram_launches + res.fused_passes
    rec = {"program": label, "qubits": n, "ops": len(prog["ops"]), "rounds": res.n_rounds,
           "fused_passes": res.fused_passes, "wall_ms": wall, "device_ms": res.device_ms,
           "histogram_ms": res.histogram_ms, "pass_ms": res.device_ms - res.histogram_ms,
           "histogram_ms_per_round": res.histogram_ms / max(1, res.n_rounds),
           "histogram_GBps": 16.0 * (1 << n) * res.histogram_launches / (res.histogram_ms * 1e6) if res.histogram_ms else None,
           "histogram_share_of_device": res.histogram_ms / res.device_ms if res.device_ms else None,
           "host_ms": res.host_ms, "host_ms_per_launch": res.host_ms / max(1, launches),
           "host_ms_per_round": res.host_ms / max(1, res.n_rounds),
           "device_ms_per_round": res.device_ms / max(1, res.n_rounds),
           "host_share_per_round": res.host_ms / res.device_ms if res.device_ms else None}
    print(json.dumps(rec), flush=True)
    return rec


def main() -> None:
    out_path = Path(sys.argv[1]) if len(sys.argv) > 1 else None
    report = {"rate_vs_norm2_30q": rate_vs_norm2(30), "runs": []}
    for n in (28, 30):
        report["runs"].append(run_one(f"bwt-style n={n}", validate_dynamic(qasm_to_dynamic(
            dynamic_bwt_style_qasm(n, n_gates=600, every=12, seed=n)))))
        report["runs"].append(run_one(f"square_root-style n={n}", validate_dynamic(qasm_to_dynamic(
            dynamic_square_root_style_qasm(n, n_blocks=8, seed=n)))))
    with tarfile.open(ROOT / "tests" / "golden" / "qasmbench_cluster.tar.xz") as tar:
        text = tar.extractfile("square_root_n30/square_root_n30.qasm").read().decode()
    report["runs"].append(run_one("square_root_n30 (QASMBench)", validate_dynamic(qasm_to_dynamic(text))))
    if out_path:
        out_path.parent.mkdir(parents=True, exist_ok=True)
        out_path.write_text(json.dumps(report, indent=1) + "\n")


if __name__ == "__main__":
    main()
