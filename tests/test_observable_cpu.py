"""Pauli sums on the host: parsing and its errors, the label order, masks under a layout, the numpy restatement of
<psi|P|psi> against explicit Kronecker products (this pins the Y phase), and the invariants of the device's pass plan
(qsim_plan_expectation: a pure function, no GPU)."""
import itertools

import numpy as np
import pytest

from quantum_simulations_amd.kernel.device import plan_expectation
from quantum_simulations_amd.observable import PauliSum, pauli_terms_np

_M = {"I": np.eye(2), "X": np.array([[0, 1], [1, 0]]), "Y": np.array([[0, -1j], [1j, 0]]), "Z": np.diag([1, -1])}


def _kron_matrix(ops: dict, n: int) -> np.ndarray:
    """Qubit q = bit q of the index: qubit 0 is the LAST factor of the Kronecker product."""
    m = np.eye(1)
    for q in reversed(range(n)):
        m = np.kron(m, _M[ops.get(q, "I")])
    return m


def test_parse_forms_agree():
    a = PauliSum([(0.5, {0: "X", 3: "Z"}), (2.0, {7: "Y"})], n_qubits=8)
    b = PauliSum({"X0 Z3": 0.5, "Y7": 2.0}, n_qubits=8)
    c = PauliSum({"YIIIZIIX": 2.0}, n_qubits=8)       # dense: rightmost character = qubit 0
    assert (a.x, a.z, list(a.coeffs)) == (b.x, b.z, list(b.coeffs))
    assert (c.x, c.z) == ([(1 << 7) | 1], [(1 << 7) | (1 << 3)])
    assert a.labels() == ["X0 Z3", "Y7"]


def test_dense_label_order_is_qiskit():
    p = PauliSum({"IXZ": 1.0})
    assert p.x == [0b010] and p.z == [0b001] and p.n_qubits == 2
    assert PauliSum({"XI": 1.0}, n_qubits=2).x == [0b10]


def test_duplicates_are_summed_and_identity():
    p = PauliSum([(1.0, {1: "Z"}), (0.25, {}), (2.0, {1: "Z"}), (0.5, "I")], n_qubits=2)
    assert len(p) == 2 and list(p.coeffs) == [3.0, 0.75]
    assert p.labels() == ["Z1", "I"]


@pytest.mark.parametrize("bad", [
    lambda: PauliSum([(1.0, {0: "Q"})], n_qubits=2),              # bad letter
    lambda: PauliSum({"X0 Z0": 1.0}, n_qubits=2),                  # repeated qubit
    lambda: PauliSum({"X5": 1.0}, n_qubits=4),                     # qubit >= n
    lambda: PauliSum({"Z1": 1 + 2j}, n_qubits=4),                  # complex coefficient
    lambda: PauliSum({"ABZ": 1.0}),                                # bad dense letter
    lambda: PauliSum([(1.0, {-1: "X"})], n_qubits=2),              # negative qubit
    lambda: PauliSum({"Z0": "x"}, n_qubits=2),                     # not a number
])
def test_rejects(bad):
    with pytest.raises(ValueError):
        bad()


def test_real_complex_coefficient_accepted():
    assert list(PauliSum({"Z0": 1.5 + 0j}).coeffs) == [1.5]


def test_masks_under_a_layout():
    p = PauliSum({"X0 Y1 Z2": 1.0, "Z3": 1.0}, n_qubits=4)
    l2p = [2, 0, 3, 1]
    x, z = p.masks(l2p)
    assert list(x) == [(1 << 2) | (1 << 0), 0]
    assert list(z) == [(1 << 0) | (1 << 3), 1 << 1]
    x0, z0 = p.masks()
    assert list(x0) == [0b011, 0] and list(z0) == [0b110, 0b1000]
    with pytest.raises(ValueError):
        p.masks([0, 0, 1, 2])


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_formula_against_kron_for_every_string(n):
    rng = np.random.default_rng(n)
    psi = rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)
    for letters in itertools.product("IXYZ", repeat=n):
        ops = {q: letters[q] for q in range(n) if letters[q] != "I"}
        p = PauliSum([(1.0, ops)], n_qubits=n)
        want = np.vdot(psi, _kron_matrix(ops, n) @ psi)
        assert abs(want.imag) < 1e-12
        got = pauli_terms_np(psi, p.x, p.z)[0]
        assert abs(got - want.real) < 1e-12, (letters, got, want)


def test_operator_reference_against_the_parity_formula_and_kron():
    """tests/pauli_reference.py (P applied to the reshaped state: the host reference of the GPU tests at 2^22 amplitudes)
    against pauli_terms_np on a 10-qubit random state, over the single-qubit and random strings the GPU suite uses, and
    P |psi> itself against the explicit Kronecker matrix for every string on 3 qubits (the Y phase and the axis order)."""
    from tests.pauli_reference import apply_pauli, pauli_terms_operator
    from tests.test_gpu_expectation import _terms
    n = 10
    rng = np.random.default_rng(10)
    psi = rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)
    psi /= np.linalg.norm(psi)
    x, z = _terms(n, 110)
    assert len(x) == 1 + 3 * n + 3 * n
    got, want = pauli_terms_operator(psi, x, z), pauli_terms_np(psi, x, z)
    # both are double sums of 2^10 products whose moduli add up to at most 1 (Cauchy-Schwarz): each within 2^10 eps = 1.1e-13
    assert float(np.max(np.abs(got - want))) < 2.5e-13, int(np.argmax(np.abs(got - want)))
    assert float(np.max(np.abs(want[1:]))) > 1e-3                   # (not a comparison of zeros)
    phi = rng.standard_normal(8) + 1j * rng.standard_normal(8)
    for letters in itertools.product("IXYZ", repeat=3):
        ops = {q: letters[q] for q in range(3) if letters[q] != "I"}
        p = PauliSum([(1.0, ops)], n_qubits=3)
        np.testing.assert_allclose(apply_pauli(phi, p.x[0], p.z[0]), _kron_matrix(ops, 3) @ phi, rtol=0, atol=1e-15)
    with pytest.raises(ValueError):
        apply_pauli(phi, 1 << 3, 0)


def test_value_applies_coefficients_in_order():
    p = PauliSum({"Z0": 2.0, "X1": -0.5}, n_qubits=2)
    assert p.value([0.25, 1.0]) == 2.0 * 0.25 - 0.5
    with pytest.raises(ValueError):
        p.value([1.0])


# ---- qsim_plan_expectation --------------------------------------------------------------------------------
def _check_plan(k, x):
    pass_of, tiles = plan_expectation(k, x)
    assert len(pass_of) == len(x)
    line = (1 << min(k, 3)) - 1
    counts = np.bincount(pass_of, minlength=len(tiles)) if len(x) else np.zeros(0, int)
    assert all(c >= 1 for c in counts)                       # no empty pass
    assert all(c <= 1024 for c in counts)
    seen_wide = False
    for p, t in enumerate(tiles):
        t = int(t)
        if t == 0 and k > 0:
            seen_wide = True
            assert counts[p] == 1
        else:
            assert not seen_wide                              # wide-X passes come last
            assert bin(t).count("1") == min(k, 11) and t & line == line and t >> k == 0
    for xi, p in zip(x, pass_of):
        t = int(tiles[p])
        if t or k == 0:
            assert int(xi) & ~t == 0                          # x inside the tile
        else:
            assert bin(int(xi) | line).count("1") > min(k, 11)   # wide only when it does not fit
    return pass_of, tiles


def test_plan_all_z_is_one_pass():
    for n_terms in (1, 17, 435, 1024):
        pass_of, tiles = _check_plan(30, np.zeros(n_terms, dtype=np.uint64))
        assert len(tiles) == 1 and not pass_of.any()
    pass_of, tiles = _check_plan(30, np.zeros(1025, dtype=np.uint64))   # over the cap: one more pass
    assert len(tiles) == 2 and list(np.bincount(pass_of)) == [1024, 1]


def test_plan_heisenberg_chain_30():
    x = []
    for a in range(29):
        pair = (1 << a) | (1 << (a + 1))
        x += [pair, pair, 0]                                  # XX, YY, ZZ
    pass_of, tiles = _check_plan(30, np.array(x, dtype=np.uint64))
    assert len(tiles) <= 6


def test_plan_term_order_and_determinism():
    rng = np.random.default_rng(5)
    x = np.array([int(sum(1 << int(b) for b in rng.choice(30, size=rng.integers(0, 5), replace=False)))
                  for _ in range(1000)], dtype=np.uint64)
    a = _check_plan(30, x)
    b = _check_plan(30, x)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    # first fit: the first term with x != 0 opens pass 0
    first = int(np.flatnonzero(x)[0])
    assert a[0][first] == 0


def test_plan_wide_terms_and_small_chunks():
    k = 20
    wide = (1 << 20) - 1                                      # X on every bit
    x = np.array([0, wide, 1 << 19, (0b11111111 << 11), (0b111111111 << 11)], dtype=np.uint64)   # 8 + 3 line bits fit, 9 + 3 do not
    pass_of, tiles = _check_plan(k, x)
    assert [int(tiles[pass_of[i]]) == 0 for i in range(5)] == [False, True, False, False, True]
    for k in range(0, 12):                                     # a chunk of <= 2^11 amplitudes: one tile holds it all
        x = np.array([(1 << k) - 1, 0, 1 if k else 0], dtype=np.uint64)
        pass_of, tiles = _check_plan(k, x)
        assert len(tiles) == 1


def test_plan_rejects_nonlocal_bit():
    with pytest.raises(NotImplementedError):
        plan_expectation(10, np.array([1 << 10], dtype=np.uint64))
