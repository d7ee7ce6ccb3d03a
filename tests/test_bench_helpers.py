"""bench.py's bookkeeping that does not need a GPU: the PMC traffic figure is taken only from a summary made with the
kernel sources of the running build (a stale figure must not look live), at the right shard size."""
import importlib
import json
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent


def _bench():
    sys.path.insert(0, str(ROOT))
    return importlib.import_module("bench")


def test_traffic_only_from_a_summary_of_the_same_sources(tmp_path, monkeypatch):
    bench = _bench()
    from quantum_simulations_amd._lib import source_hash
    prof = tmp_path / "profiles"
    prof.mkdir()
    monkeypatch.setattr(bench, "ROOT", tmp_path)
    row = {"kernel": "k_tile", "hbm_bytes_per_launch": 8.59e9}
    (prof / "r01_pmc_summary.json").write_text(json.dumps({"csrc_sha16": "0123456789abcdef", "kernels": [row]}))
    assert bench.pmc_traffic_per_launch("k_tile") == (None, None)                       # stale: other sources
    (prof / "r02_pmc_summary.json").write_text(json.dumps({"kernels": [row]}))           # no hash at all (round 2 files)
    assert bench.pmc_traffic_per_launch("k_tile") == (None, None)
    (prof / "r03_pmc_summary.json").write_text(json.dumps({"csrc_sha16": source_hash(), "kernels": [row]}))
    assert bench.pmc_traffic_per_launch("k_tile") == (8.59e9, "profiles/r03_pmc_summary.json")
    assert bench.pmc_traffic_per_launch("k_gate") == (None, None)                       # another kernel
    assert bench.pmc_traffic_per_launch("k_tile", 30) == (None, None)                   # another shard size
    (prof / "r03b_pmc_summary.json").write_text(json.dumps({"csrc_sha16": source_hash(), "local_qubits": 30,
                                                             "kernels": [dict(row, hbm_bytes_per_launch=3.436e10)]}))
    assert bench.pmc_traffic_per_launch("k_tile", 30) == (3.436e10, "profiles/r03b_pmc_summary.json")
    assert bench.pmc_traffic_per_launch("k_tile", 28)[0] == 8.59e9
    (prof / "broken_pmc_summary.json").write_text("{not json")
    assert bench.pmc_traffic_per_launch("k_tile", 28)[0] == 8.59e9


def test_the_committed_summaries_match_the_committed_sources():
    """The judged profiles of the round were taken with the sources in the tree: bench.py will print their traffic."""
    from quantum_simulations_amd._lib import source_hash
    now = source_hash()
    docs = [json.loads(p.read_text()) for p in (ROOT / "profiles").glob("*_pmc_summary.json")]
    live = [d for d in docs if d.get("csrc_sha16") == now]
    if not {d.get("local_qubits", 28) for d in live} >= {28, 30}:
        import pytest
        pytest.skip("profiles/*_pmc_summary.json are older than csrc/: bench.py prints traffic = null until "
                    "tools/profile_round.sh has run on the GPU with these sources")


def test_probe_environment_is_refused(monkeypatch):
    bench = _bench()
    import pytest
    monkeypatch.setenv("QSIM_PLAN_LOOKAHEAD", "0")
    with pytest.raises(SystemExit) as e:
        bench.refuse_probe_environment()
    assert e.value.code == 2
    monkeypatch.delenv("QSIM_PLAN_LOOKAHEAD")
    monkeypatch.setenv("QSIM_DIST_BACKEND", "gloo")     # round 3's rehearsal switch: now an explicit flag (--rehearsal),
    with pytest.raises(SystemExit):                     # no environment variable changes what a bench line means
        bench.refuse_probe_environment()
    monkeypatch.delenv("QSIM_DIST_BACKEND")
    bench.refuse_probe_environment()


class _HostEngine:
    """The two things dump_outputs reads of an engine: `l2p` and `state.download(offset, count)`, over a host array that
    holds a logical state in the layout l2p (logical qubit q on index bit l2p[q])."""

    def __init__(self, psi_logical, l2p):
        self.n = int(psi_logical.size).bit_length() - 1
        self.l2p = l2p
        phys = np.arange(psi_logical.size)
        if l2p is not None:
            logical = np.zeros_like(phys)
            for q, p in enumerate(l2p):
                logical |= ((phys >> p) & 1) << q
            phys = logical
        held = psi_logical[phys]
        self.state = type("S", (), {"download": staticmethod(lambda off, cnt: held[off:off + cnt].copy())})()


def test_dump_outputs_undoes_the_layout_and_samples_the_same_indices(tmp_path, monkeypatch):
    bench = _bench()
    rng = np.random.default_rng(5)
    n = 12
    psi = rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)
    l2p = list(rng.permutation(n))
    rec = bench.dump_outputs(_HostEngine(psi, l2p), tmp_path / "a")          # whole state
    got = np.load(tmp_path / "a" / "state.npy")
    assert got.dtype == np.float64 and got.shape == (1 << n, 2) and rec["sample"] is None
    np.testing.assert_array_equal(got[:, 0] + 1j * got[:, 1], psi)
    monkeypatch.setattr(bench, "DUMP_MAX_AMPLITUDES", 1 << 9)                 # sampled: fixed indices, same in every run
    bench.dump_outputs(_HostEngine(psi, l2p), tmp_path / "b")
    bench.dump_outputs(_HostEngine(psi, None), tmp_path / "c")
    b, c = np.load(tmp_path / "b" / "state.npy"), np.load(tmp_path / "c" / "state.npy")
    idx = np.unique(np.random.default_rng(bench.DUMP_SEED).integers(0, 1 << n, size=1 << 9, dtype=np.int64))
    np.testing.assert_array_equal(b, c)
    np.testing.assert_array_equal(b[:, 0] + 1j * b[:, 1], psi[idx])


def test_steps_and_warmup_are_checked(monkeypatch):
    bench = _bench()
    for argv in (["--steps", "0"], ["--warmup", "-1"]):
        monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
        with pytest.raises(SystemExit):
            bench.parse_args()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "7", "--warmup", "2"])
    args = bench.parse_args()
    assert args.steps == 7 and args.warmup == 2 and not args.full and args.dump_outputs is None
