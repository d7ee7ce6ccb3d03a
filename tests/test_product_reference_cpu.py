"""tests/product_reference.py against dense vectors and explicit Kronecker matrices at n = 6 .. 10 (no GPU).  Bound 1e-13 on
unit-norm states: every closed form is a product of n factors and a sum of at most a few hundred terms, evaluated in long
double, and the dense side is a handful of double-precision matrix products; a prototype of the Pauli, overlap and CDF
forms at n = 8 gave 6.5e-17, 2.8e-16 and no failing shot."""
import numpy as np
import pytest

from tests import diagonal_reference as dref
from tests import product_reference as ref
from tests.rdm_reference import rdm_np

ATOL = 1e-13
SIZES = [6, 7, 8, 9, 10]
_I = np.eye(2, dtype=np.complex128)
_X = np.array([[0, 1], [1, 0]], dtype=np.complex128)
_Y = np.array([[0, -1j], [1j, 0]], dtype=np.complex128)
_Z = np.diag([1.0, -1.0]).astype(np.complex128)


def dense(f):
    """The Kronecker product of the factors, the highest qubit leftmost: qubit q is index bit q."""
    v = np.ones(1, dtype=np.complex128)
    for q in reversed(range(len(f))):
        v = np.kron(v, f[q])
    return v


def dense_sum(ps):
    return sum(c * dense(f) for c, f in ps)


def kron_pauli(n, x, z):
    m = np.ones((1, 1), dtype=np.complex128)
    for q in reversed(range(n)):
        bx, bz = (x >> q) & 1, (z >> q) & 1
        m = np.kron(m, _Y if bx and bz else _X if bx else _Z if bz else _I)
    return m


def _strings(n, seed, count):
    rng = np.random.default_rng(seed)
    full = (1 << n) - 1
    fixed = [(0, 0), (full, 0), (full, full), (0, full), (1 << (n - 1), 0), (1 << (n - 1), 1 << (n - 1)), (1, 1 << (n - 1))]
    return fixed + [(int(rng.integers(0, full + 1)), int(rng.integers(0, full + 1))) for _ in range(count)]


def _err(got, want):
    return float(np.max(np.abs(np.asarray(got) - np.asarray(want))))


@pytest.mark.parametrize("n", SIZES)
def test_factors_amplitudes_and_state_ops(n):
    f, g = ref.factors(n, n), ref.factors(n, n, near=50 + n)
    assert f.shape == g.shape == (n, 2)
    for h in (f, g):
        assert _err(np.sum(np.abs(h) ** 2, axis=1), 1.0) < 1e-15
        polar = 2.0 * np.arctan2(np.abs(h[:, 1]), np.abs(h[:, 0]))
        assert np.all(polar > 0.3 - 1e-12) and np.all(polar < np.pi - 0.3 + 1e-12)
    assert 0.0 < _err(np.angle(g[:, 1] / f[:, 1]), 0.0) <= 0.2 + 1e-12         # the perturbed state is near, not equal
    idx = np.arange(1 << n, dtype=np.uint64)
    assert _err(ref.amplitudes(f, idx), dense(f)) < ATOL
    assert np.min(np.abs(dense(f))) > 0.0
    some = np.array([[0, 5], [(1 << n) - 1, 17]], dtype=np.uint64)             # any shape of indices
    assert _err(ref.amplitudes(f, some), dense(f)[some.astype(np.int64)]) < ATOL
    psi = np.zeros(1 << n, dtype=np.complex128)
    psi[0] = 1.0
    for (q,), U in ref.state_ops(f):
        assert _err(U.conj().T @ U, _I) < 1e-15 and _err(U[:, 0], f[q]) == 0.0
        psi = np.moveaxis(np.tensordot(U, psi.reshape([2] * n), axes=([1], [n - 1 - q])), 0, n - 1 - q).reshape(-1)
    assert _err(psi, dense(f)) < ATOL
    assert abs(ref.inner([(1.0, g)], [(1.0, f)])) > 0.5                         # <phi|psi> is O(1)


@pytest.mark.parametrize("n", SIZES)
def test_pauli_on_against_kronecker_matrices(n):
    f = ref.factors(n, 10 + n)
    psi = dense(f)
    worst = 0.0
    for x, z in _strings(n, 20 + n, 12):
        worst = max(worst, _err(dense(ref.pauli_on(f, x, z)), kron_pauli(n, x, z) @ psi))
    print(f"n={n}: pauli_on, max |closed form - dense| = {worst:.3e} (bound {ATOL:g})")
    assert worst < ATOL
    with pytest.raises(ValueError):
        ref.pauli_on(f, 1 << n, 0)


def _four_rotations(n):
    """Each does not commute with the one before it."""
    top = 1 << (n - 1)
    rots = [(0b110, top | 0b100, 0.7), (top | 0b11, 0, -1.1), (0, top | (1 << (n - 2)) | 0b11, 0.45), ((1 << n) - 1 - 0b1010, 0b101, 2.3)]
    for (x1, z1, _), (x2, z2, _) in zip(rots[:-1], rots[1:]):
        assert not ref.commute(x1, z1, x2, z2)
    return rots


@pytest.mark.parametrize("n", SIZES)
def test_product_sum_after_four_non_commuting_rotations(n):
    f, g = ref.factors(n, 30 + n), ref.factors(n, 30 + n, near=60 + n)
    ps, psi = [(1.0, f)], dense(f)
    for x, z, th in _four_rotations(n):
        ps = ref.rotate(ps, x, z, th)
        psi = np.cos(th) * psi - 1j * np.sin(th) * (kron_pauli(n, x, z) @ psi)
    assert len(ps) == 16
    idx = np.arange(1 << n, dtype=np.uint64)
    e_amp = _err(ref.sum_amplitudes(ps, idx), psi)
    e_norm = abs(ref.inner(ps, ps) - 1.0)
    e_ovl = abs(ref.inner([(1.0, g)], ps) - np.vdot(dense(g), psi))
    e_exp = max(abs(ref.expectation(ps, x, z) - np.vdot(psi, kron_pauli(n, x, z) @ psi).real) for x, z in _strings(n, 40 + n, 6))
    print(f"n={n}: 16-term ProductSum: amplitudes {e_amp:.3e}, norm {e_norm:.3e}, overlap {e_ovl:.3e}, expectation {e_exp:.3e} (bound {ATOL:g})")
    assert max(e_amp, e_norm, e_ovl, e_exp) < ATOL
    # the order matters, and the closed form knows it
    back = [(1.0, f)]
    for x, z, th in reversed(_four_rotations(n)):
        back = ref.rotate(back, x, z, th)
    assert _err(ref.sum_amplitudes(back, idx), psi) > 1e-3


@pytest.mark.parametrize("n", SIZES)
def test_inner_and_apply_sum(n):
    rng = np.random.default_rng(70 + n)
    a = [(complex(rng.standard_normal(), rng.standard_normal()), ref.factors(n, 80 + n + j)) for j in range(3)]
    b = [(complex(rng.standard_normal(), rng.standard_normal()), ref.factors(n, 90 + n + j)) for j in range(2)]
    assert abs(ref.inner(a, b) - np.vdot(dense_sum(a), dense_sum(b))) < ATOL
    assert abs(ref.inner(b, a) - np.conj(ref.inner(a, b))) < 1e-15
    strings = _strings(n, 100 + n, 5)
    xs, zs = [s[0] for s in strings], [s[1] for s in strings]
    co = rng.standard_normal(len(strings))
    co /= np.sum(np.abs(co))
    f = ref.factors(n, 110 + n)
    h = ref.apply_sum([(1.0, f)], xs, zs, co)
    want = sum(c * (kron_pauli(n, x, z) @ dense(f)) for x, z, c in zip(xs, zs, co))
    assert _err(dense_sum(h), want) < ATOL
    assert abs(ref.inner(h, h) - np.vdot(want, want)) < ATOL
    for x, z in strings:                                                        # <g|P|f>, the two-state matrix element
        g = ref.factors(n, 120 + n)
        assert abs(ref.inner([(1.0, g)], [(1.0, ref.pauli_on(f, x, z))]) - np.vdot(dense(g), kron_pauli(n, x, z) @ dense(f))) < ATOL


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("r", [1, 3, 6])
def test_rdm(n, r):
    f = ref.factors(n, 130 + n)
    ps = ref.rotate([(1.0, f)], (1 << (n - 1)) | 1, (1 << (n - 2)) | 0b100, 0.6)     # entangles the ends
    qubits = [n - 1, 0, 2, n - 2, 3, 1][:r]
    got = ref.rdm(ps, qubits)
    err = _err(got, rdm_np(dense_sum(ps), qubits))
    print(f"n={n} r={r}: rdm max |closed form - dense| = {err:.3e} (bound {ATOL:g})")
    assert err < ATOL
    assert abs(np.trace(got) - 1.0) < ATOL and _err(got, got.conj().T) < 1e-15
    if r == 1:
        assert abs(np.trace(got @ got).real - 1.0) > 1e-3                      # a mixed state: the rotation entangled
    if r == n:                                                                  # nothing traced out: |psi><psi| in the order of `qubits`
        psi = dense_sum(ps).reshape([2] * n).transpose([n - 1 - q for q in reversed(qubits)]).reshape(-1)
        assert _err(got, np.outer(psi, psi.conj())) < ATOL


@pytest.mark.parametrize("n", SIZES)
def test_diagonal_energy_phase_and_moments(n):
    rng = np.random.default_rng(140 + n)
    z = rng.integers(0, 1 << n, 300).astype(np.uint64)
    z[:3] = [0, (1 << n) - 1, 1 << (n - 1)]
    z[10] = z[11]                                                               # a duplicate
    gamma = -1.3
    co = rng.standard_normal(300)
    co *= 32.0 / (abs(gamma) * np.sum(np.abs(co)))
    idx = np.arange(1 << n, dtype=np.uint64)
    weight = float(np.sum(np.abs(co)))
    e = ref.diag_energy(idx, z, co)
    assert _err(e.astype(np.float64), dref.energies_naive(n, z, co)) / weight < ATOL
    zdiag = [np.real(np.diag(kron_pauli(n, 0, int(m)))) for m in z[:8]]         # against Kronecker matrices of Z
    assert _err(ref.diag_energy(idx, z[:8], co[:8]).astype(np.float64), sum(c * d for c, d in zip(co[:8], zdiag))) / weight < ATOL
    f = ref.factors(n, 150 + n)
    psi = dense(f)
    assert _err(ref.amplitudes(f, idx) * ref.diag_phase(idx, z, co, gamma), dref.phase(psi, z, co, gamma)) < ATOL
    got, want = ref.diag_moments(f, z, co), dref.moments(psi, z, co)
    errs = (abs(got[0] - want[0]), abs(got[1] - want[1]) / weight, abs(got[2] - want[2]) / weight ** 2)
    print(f"n={n}: moments of 300 terms, |closed form - dense| = {errs[0]:.2e}, {errs[1]:.2e}, {errs[2]:.2e} (bound {ATOL:g})")
    assert max(errs) < ATOL
    assert ref.diag_moments(f, [], [])[1:] == (0.0, 0.0)
    # a short sum as rotations: exp(-i gamma D) psi is a ProductSum
    ps = [(1.0, f)]
    for zt, ct in zip(z[:4], co[:4]):
        ps = ref.rotate(ps, 0, int(zt), gamma * ct)
    assert _err(ref.sum_amplitudes(ps, idx), dref.phase(psi, z[:4], co[:4], gamma)) < ATOL


@pytest.mark.parametrize("n", SIZES)
def test_cdf_interval_against_a_long_double_cumsum(n):
    f = ref.factors(n, 160 + n)
    psi = dense(f)
    p = psi.real.astype(ref.LD) ** 2 + psi.imag.astype(ref.LD) ** 2
    P = np.cumsum(p)
    idx = np.arange(1 << n, dtype=np.uint64)
    below, here = ref.cdf_interval(f, idx)
    e_below = float(np.max(np.abs(below - np.concatenate([[0], P[:-1]]))))
    e_here = float(np.max(np.abs(here - p)))
    print(f"n={n}: cdf_interval against cumsum: below {e_below:.3e}, p {e_here:.3e} (bound {ATOL:g})")
    assert e_below < ATOL and e_here < ATOL
    assert below[0] == 0 and abs(float(below[-1] + here[-1]) - 1.0) < ATOL


@pytest.mark.parametrize("n", [8, 10])
def test_sampling_criterion_from_cdf_interval(n):
    """20 000 uniforms located in the long-double cumulative sum of the dense state (an inverse CDF that shares nothing
    with cdf_interval): no shot may miss the criterion; the neighbouring index of every shot does."""
    f = ref.factors(n, 170 + n)
    psi = dense(f)
    P = np.cumsum(psi.real.astype(ref.LD) ** 2 + psi.imag.astype(ref.LD) ** 2)
    r = np.concatenate([np.random.default_rng(180 + n).random(20000), [0.0, np.nextafter(1.0, 0.0), 0.5]])
    idx = np.minimum(np.searchsorted(P, r.astype(ref.LD) * P[-1], side="right"), (1 << n) - 1).astype(np.uint64)
    bad = ref.shot_failures(f, r, idx)
    assert bad.size == 0, (bad[:5], idx[bad[:5]], r[bad[:5]])
    assert idx[-3] == 0 and idx[-2] == (1 << n) - 1
    off = (idx + np.uint64(1)) % np.uint64(1 << n)
    assert ref.shot_failures(f, r, off).size > 0.99 * r.size
    with pytest.raises(AssertionError):
        ref.shot_failures(f, r[:2], np.array([0, 1 << n], dtype=np.uint64))


def test_windows():
    for n, special in ((29, [(1 << 28) - 2048]), (32, [(1 << 28) - 2048, (1 << 31) - 2048, (1 << 32) - 4096]), (14, [])):
        w = ref.windows(n)
        offs = [o for o, _ in w]
        assert all(c == ref.WINDOW for _, c in w) and offs == sorted(set(offs))
        assert offs[0] == 0 and offs[-1] == (1 << n) - ref.WINDOW and all(s in offs for s in special)
        assert all(0 <= o and o + c <= 1 << n for o, c in w)
        upper = [o for o in offs if o >= 1 << (n - 1) and o % ref.WINDOW == 0 and o != offs[-1]]
        assert upper, n                                                           # the seeded aligned one
        assert ref.windows(n) == w
    assert len(ref.windows(29)) == 4 and len(ref.windows(32)) == 6
