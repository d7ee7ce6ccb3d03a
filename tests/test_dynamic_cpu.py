"""Dynamic programs without a GPU: the QASM front-end for reset / measure / if (circuit/import_qasm.qasm_to_dynamic),
the program type and its rounds (circuit/dynamic.py), the sampling rule (runner/dynamic.sample_outcome) and the
numpy oracle the GPU tests compare against (tests/dynamic_oracle.py)."""
import math
import tarfile
from pathlib import Path

import numpy as np
import pytest

from oracle import dense_oracle as orc
from quantum_simulations_amd.circuit.dynamic import MAX_ROUND_QUBITS, rounds, validate_dynamic
from quantum_simulations_amd.circuit.import_qasm import qasm_to_dict, qasm_to_dynamic
from quantum_simulations_amd.runner.dynamic import collapse_factors, sample_outcome
from tests import dynamic_oracle

HDR = 'OPENQASM 2.0;\ninclude "qelib1.inc";\n'
TARBALL = Path(__file__).resolve().parent / "golden" / "qasmbench_cluster.tar.xz"


def _members():
    with tarfile.open(TARBALL) as tar:
        members = sorted((m for m in tar.getmembers() if m.isfile() and m.name.endswith(".qasm")), key=lambda m: m.name)
        return [(Path(m.name).parent.name, tar.extractfile(m).read().decode()) for m in members]


# ---------------------------------------------------------------- front-end
def test_reset_and_measure_forms():
    p = qasm_to_dynamic(HDR + "qreg q[3]; creg c[3]; h q[0]; measure q[0] -> c[0]; reset q; x q[1]; measure q -> c;",
                        keep_terminal_measure=True)
    assert p["number_of_qubits"] == 3 and p["cregs"] == {"c": 3}
    ops = p["ops"]
    assert ops[0] == {"qubits": [0], "gate": "H", "params": {}}
    assert ops[1] == {"op": "measure", "qubit": 0, "clbit": ["c", 0]}
    assert ops[2:5] == [{"op": "reset", "qubit": q} for q in range(3)]
    assert ops[5]["gate"] == "X"
    assert ops[6:] == [{"op": "measure", "qubit": q, "clbit": ["c", q]} for q in range(3)]
    validate_dynamic(p)


def test_terminal_measures_dropped_unless_kept():
    src = HDR + ("qreg q[3]; creg c[2]; creg d[1]; h q[0]; measure q[0] -> c[0]; measure q[2] -> d[0]; "
                 "if(c==1) x q[1]; measure q[0] -> c[0]; measure q[1] -> c[1];")
    p = qasm_to_dynamic(src)
    kinds = [o.get("op", o.get("gate")) for o in p["ops"]]
    # q[0] -> c[0] is read by the if: kept; q[2] -> d[0] (nothing follows on q[2], nobody reads d) and the last two
    # are terminal
    assert kinds == ["H", "measure", "X"]
    assert p["ops"][1]["qubit"] == 0
    assert p["ops"][2]["condition"] == {"creg": "c", "value": 1}
    kept = qasm_to_dynamic(src, keep_terminal_measure=True)
    assert [o.get("op", o.get("gate")) for o in kept["ops"]] == ["H", "measure", "measure", "X", "measure", "measure"]
    # a later reset on the measured qubit makes the measurement mid-circuit
    p2 = qasm_to_dynamic(HDR + "qreg q[1]; creg c[1]; h q[0]; measure q[0] -> c[0]; reset q[0]; h q[0];")
    assert [o.get("op", o.get("gate")) for o in p2["ops"]] == ["H", "measure", "reset", "H"]


def test_if_on_single_user_and_ccx_gates():
    src = HDR + ("gate foo a,b { h a; cx a,b; }\nqreg q[3]; creg c[2]; h q[0]; measure q[0] -> c[1];"
                 "if(c==2) z q[2]; if(c==2) foo q[0],q[1]; if(c==3) ccx q[0],q[1],q[2];")
    ops = qasm_to_dynamic(src)["ops"]
    cond = [o for o in ops if "condition" in o]
    want = qasm_to_dict(HDR + "qreg q[3]; z q[2]; h q[0]; cx q[0],q[1]; ccx q[0],q[1],q[2];")["gates"]
    assert [{k: v for k, v in o.items() if k != "condition"} for o in cond] == want
    assert [o["condition"]["value"] for o in cond] == [2] * 3 + [3] * (len(want) - 3)
    assert all(o["condition"]["creg"] == "c" for o in cond)
    validate_dynamic(qasm_to_dynamic(src))


@pytest.mark.parametrize("body", ["measure q[0] -> c[0]", "reset q[0]"])
def test_if_around_measure_or_reset_rejected(body):
    with pytest.raises(ValueError, match="unsupported gate"):
        qasm_to_dynamic(HDR + f"qreg q[1]; creg c[1]; if(c==1) {body};")


def test_qasm_to_dict_still_rejects_dynamic_statements():
    for body in ("reset q[0];", "if(c==1) x q[0];", "measure q[0] -> c[0]; x q[0];"):
        with pytest.raises(ValueError, match="unsupported gate"):
            qasm_to_dict(HDR + "qreg q[1]; creg c[1]; " + body)


def test_qasmbench_inputs_import_as_dynamic_programs():
    members = _members()
    assert len(members) == 55
    plain = 0
    for name, text in members:
        prog = validate_dynamic(qasm_to_dynamic(text))
        try:
            cd = qasm_to_dict(text)
        except ValueError as e:
            assert "unsupported gate" in str(e)
            cd = None
        if cd is not None:
            plain += 1
            assert prog["ops"] == cd["gates"], name
            assert all(s["kind"] == "gates" for s in rounds(prog)), name
        elif name == "square_root_n27":
            steps = rounds(prog)
            assert sum(o.get("op") == "reset" for o in prog["ops"]) == 280
            assert sum(s["kind"] == "round" for s in steps) == 35
        elif name == "cc_n28":
            steps = rounds(prog)
            assert sum(s["kind"] == "round" for s in steps) == 1
            assert sum("condition" in o for o in prog["ops"]) == 57
    assert plain == 51


# ---------------------------------------------------------------- rounds
def _m(q, c="c"):
    return {"op": "measure", "qubit": q, "clbit": [c, q]}


def test_rounds_cut_at_eight_qubits_and_at_a_repeated_qubit():
    n = 12
    prog = validate_dynamic({"number_of_qubits": n, "cregs": {"c": n}, "ops": [_m(q) for q in range(10)]})
    st = rounds(prog)
    assert [s["qubits"] for s in st] == [list(range(8)), [8, 9]]
    assert MAX_ROUND_QUBITS == 8
    prog = validate_dynamic({"number_of_qubits": n, "cregs": {"c": n},
                             "ops": [_m(0), {"op": "reset", "qubit": 1}, _m(2), {"op": "reset", "qubit": 0}, _m(3)]})
    assert [s["qubits"] for s in rounds(prog)] == [[0, 1, 2], [0, 3]]


def test_rounds_split_by_a_conditional_gate():
    ops = [_m(0), {"qubits": [1], "gate": "X", "params": {}, "condition": {"creg": "c", "value": 1}}, _m(1)]
    st = rounds(validate_dynamic({"number_of_qubits": 2, "cregs": {"c": 2}, "ops": ops}))
    assert [s["kind"] for s in st] == ["round", "gates", "round"]
    assert st[1]["ops"][0]["condition"] == {"creg": "c", "value": 1}


def test_validate_dynamic_rejects_bad_ops():
    base = {"number_of_qubits": 2, "cregs": {"c": 2}}
    for bad in ({"op": "measure", "qubit": 0, "clbit": ["d", 0]}, {"op": "measure", "qubit": 5, "clbit": ["c", 0]},
                {"op": "reset", "qubit": 0, "clbit": ["c", 0]}, {"op": "swap", "qubit": 0},
                {"qubits": [0], "gate": "X", "params": {}, "condition": {"creg": "c", "value": 4}},
                {"qubits": [0], "gate": "NOPE", "params": {}}):
        with pytest.raises(ValueError):
            validate_dynamic({**base, "ops": [bad]})


# ---------------------------------------------------------------- sampling rule and collapse factors
def test_sampling_rule_on_given_histograms():
    p = np.array([0.0, 0.25, 0.0, 0.0, 0.5, 0.25, 0.0, 0.0])
    for u in np.linspace(0.0, 1.0, 1001, endpoint=False):
        m = sample_outcome(p, u)
        assert p[m] > 0
        c = np.cumsum(p)
        assert c[m] > u * p.sum() and (m == 0 or c[m - 1] <= u * p.sum())
    assert sample_outcome(p, 0.0) == 1                        # u = 0: the first bin with weight
    assert sample_outcome(p, 0.25) == 4                       # exactly on a boundary: the next bin
    assert sample_outcome(p, np.nextafter(1.0, 0.0)) == 5     # largest u: the last bin with weight
    assert sample_outcome(np.array([0.0, 0.0, 3.0, 0.0]), np.nextafter(1.0, 0.0)) == 2   # unnormalised


def test_collapse_factors():
    ops = [_m(2), {"op": "reset", "qubit": 5}]
    f = collapse_factors(ops, [2, 5], outcome=0b11, scale=3.0)
    assert f[0][0] == [2] and np.array_equal(f[0][1], np.array([[0, 0], [0, 3.0]]))
    assert f[1][0] == [5] and np.array_equal(f[1][1], np.array([[0, 1.0], [0, 0]]))
    f = collapse_factors(ops, [2, 5], outcome=0, scale=2.0)
    assert np.array_equal(f[0][1], np.diag([2.0, 0])) and np.array_equal(f[1][1], np.diag([1.0, 0]))


# ---------------------------------------------------------------- oracle sanity
TELEPORT = HDR + """qreg q[3]; creg a[1]; creg b[1];
ry(0.7) q[0]; rz(1.1) q[0];
h q[1]; cx q[1],q[2];
cx q[0],q[1]; h q[0];
measure q[0] -> a[0]; measure q[1] -> b[0];
if(b==1) x q[2]; if(a==1) z q[2];
"""


def test_oracle_teleportation_every_branch():
    prog = validate_dynamic(qasm_to_dynamic(TELEPORT))
    src = np.zeros(2, dtype=np.complex128)
    src[0] = 1.0
    for g in qasm_to_dict(HDR + "qreg q[1]; ry(0.7) q[0]; rz(1.1) q[0];")["gates"]:
        orc.apply_1q(src, 0, orc.gate_matrix(g["gate"], g["params"]))
    seen = set()
    for outcome in range(4):
        out = dynamic_oracle.run(prog, seed=0, forced=[outcome])
        psi = out["state"].reshape(2, 2, 2)        # [q2][q1][q0]
        m0, m1 = outcome & 1, outcome >> 1
        target = psi[:, m1, m0]
        assert abs(np.linalg.norm(psi) - 1) < 1e-14
        assert np.allclose(target, src, atol=1e-14, rtol=0)
        assert out["rounds"][0]["probability"] == pytest.approx(0.25, abs=1e-14)
        assert out["cregs"] == {"a": m0, "b": m1}
        seen.add(outcome)
    assert seen == {0, 1, 2, 3}


def test_oracle_reset_leaves_zero():
    src = HDR + "qreg q[3]; creg c[3]; h q; cx q[0],q[1]; ry(0.4) q[2]; reset q[1]; reset q[2];"
    prog = validate_dynamic(qasm_to_dynamic(src))
    for seed in range(6):
        out = dynamic_oracle.run(prog, seed=seed)
        p = dynamic_oracle.probabilities(out["state"], [1, 2])
        assert p[1] == 0 and p[2] == 0 and p[3] == 0
        assert math.isclose(p.sum(), 1.0, rel_tol=1e-14)
