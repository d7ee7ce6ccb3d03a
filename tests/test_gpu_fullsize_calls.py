"""The Pauli, diagonal, lincomb, RDM and sampling calls at the sizes the project runs at, on an MI355X.

n = 29 (8 GiB a chunk) is the smallest state with byte offsets past 2^32 (amplitude index >= 2^28); n = 32 (64 GiB) the
smallest with amplitude indices past 2^31.  At n = 29 a tile kernel's 1024 workgroups walk 256 tiles each, a wide kernel
makes 1024 strides, the writing form of k_lincomb launches 2^19 workgroups, and every kernel runs its non-temporal form.

No host copy: psi and phi are PRODUCT states built on the device by n one-qubit gates, and tests/product_reference.py
gives every amplitude, inner product, expectation value, density matrix, moment and CDF value in closed form (pinned
against dense numpy in tests/test_product_reference_cpu.py at 1e-13).  Amplitudes are compared in windows of 4096 at the
offsets of `product_reference.windows`: the start, the window that straddles the 4 GiB byte boundary, a seeded one in the
upper half, the ends, and at n = 32 the window across amplitude 2^31.

Bounds.  Windows: 1e-12 * max |want| over the window, the project's per-call bound made relative (amplitudes are about
4e-5 here; an absolute 1e-12 would check 8 digits).  Scalars (norms, overlaps, expectation values, density-matrix
entries: magnitude <= 1): 1e-12 absolute.  The 300-term diagonal list is scaled to |gamma| sum|c| = 32 as in
tests/test_gpu_diagonal.py, whose derived phase error of about 1e-13 stays inside the window bound; moments are relative
to sum|c| and (sum|c|)^2 as there.  Sampling: the criterion of tests/test_gpu_sampling.py with the closed-form CDF.
The state itself is checked first, so a later failure belongs to the call under test.  (The density matrix of r = 6
qubits takes the five named bits 0, 2, 11, n - 2, n - 1 and bit 20: five bits do not make six.)"""
import time

import numpy as np
import pytest

from quantum_simulations_amd import sampling
from quantum_simulations_amd.kernel.device import DeviceChunk, plan_expectation
from quantum_simulations_amd.kernel.planner import plan_pauli_rotations
from tests import product_reference as ref

pytestmark = pytest.mark.gpu

N, BIG = 29, 32
RTOL = 1e-12           # windows: relative to the largest wanted amplitude of the window
ATOL = 1e-12           # scalars of magnitude <= 1
WEIGHT = 32.0          # |gamma| sum |c_t| of the long diagonal list


def _f(n, which):
    """psi, phi (psi's angles perturbed by at most 0.2), and two unrelated product states."""
    return {"psi": ref.factors(n, 7 * n), "phi": ref.factors(n, 7 * n, near=7 * n + 1), "chi": ref.factors(n, 7 * n + 2),
            "omega": ref.factors(n, 7 * n + 3)}[which]


def _prepare(c, f):
    c.init_zero()
    c.apply_ops(ref.state_ops(f))


def _windows(c, want_of, what):
    """max over the windows of max |got - want| / max |want|, asserted below RTOL."""
    worst = 0.0
    for off, count in ref.windows(c.k):
        idx = np.arange(off, off + count, dtype=np.uint64)
        want = want_of(idx)
        got = c.download(off, count)
        scale = float(np.max(np.abs(want)))
        err = float(np.max(np.abs(got - want)))
        print(f"  {what}: window at {off}: max |got - want| = {err:.3e}, max |want| = {scale:.3e}, ratio {err / scale:.3e} (bound {RTOL:g})")
        assert scale > 0.0 and err < RTOL * scale, (what, off, err, scale)
        worst = max(worst, err / scale)
    return worst


def _window_bytes(c):
    return [c.download(off, count).tobytes() for off, count in ref.windows(c.k)]


def _scalar(got, want, what, scale=1.0):
    err = abs(got - want) / scale
    print(f"  {what}: |got - want| = {err:.3e} (bound {ATOL:g})")
    assert err < ATOL, (what, got, want)


class _Timer:
    def __init__(self, what):
        self.what = what

    def __enter__(self):
        self.t0 = time.perf_counter()

    def __exit__(self, *exc):
        print(f"{self.what}: {time.perf_counter() - self.t0:.2f} s")


@pytest.fixture(scope="module")
def chunks():
    """Three chunks of 2^29 amplitudes (24 GiB), for every n = 29 test of this file."""
    cs = [DeviceChunk.empty(N) for _ in range(3)]
    yield cs
    for c in cs:
        c.close()


@pytest.fixture(scope="module")
def big():
    """One chunk of 2^32 amplitudes (64 GiB)."""
    try:
        c = DeviceChunk.empty(BIG)
    except MemoryError:
        pytest.skip("device has less than 64 GiB free")
    yield c
    c.close()


# ---- the lists -----------------------------------------------------------------------------------------------------------
def _wide_x(n):
    """X on 14 bits, bit n - 1 among them: more than a tile holds."""
    return sum(1 << b for b in (n - 1, n - 2, 20, 17, 15, 13, 12, 11, 10, 9, 8, 6, 4, 0))


def _rotations(n):
    """Four rotations, each anticommuting with the one before: X on low bits with Z on bits >= 27; X on bit n - 1 and two
    low bits (the tile holds the top bit); Z only on {0, n - 2, n - 1}; X on 14 bits (k_rot_wide)."""
    top, sub = 1 << (n - 1), 1 << (n - 2)
    rots = [((1 << 1) | (1 << 5), (1 << 27) | top | (1 << 5), 0.7),
            (top | (1 << 3) | (1 << 7), (1 << 3) | (1 << 12), -1.1),
            (0, 1 | sub | top, 0.45),
            (_wide_x(n), (1 << 4) | (1 << 27) | (1 << 2), 2.3)]
    for (x1, z1, _), (x2, z2, _) in zip(rots[:-1], rots[1:]):
        assert not ref.commute(x1, z1, x2, z2)
    return rots


def _six_strings(n):
    top, sub = 1 << (n - 1), 1 << (n - 2)
    return [(0, top), (top, 0), (1, sub | 1), (0b1010, 1 << 27), (_wide_x(n), (1 << 4) | 1), (top | sub, top)]


def _sum_terms(n):
    """Eight terms: seven whose x fit one tile with the line bits (bits 1, 5, 12, n - 2, n - 1) and a wide one."""
    top, sub = 1 << (n - 1), 1 << (n - 2)
    return [(top, 0), (top | (1 << 1), top), (1 << 5, (1 << 27) | (1 << 5)), (0, top | sub | 1), ((1 << 12) | sub, (1 << 12) | (1 << 20)),
            (0, 0), ((1 << 1) | (1 << 5) | (1 << 12), top), (_wide_x(n), (1 << 4) | (1 << 27) | (1 << 2))]


def _masks(pairs):
    return np.array([p[0] for p in pairs], dtype=np.uint64), np.array([p[1] for p in pairs], dtype=np.uint64)


def _long_diagonal(n, seed, gamma):
    rng = np.random.default_rng(seed)
    z = rng.integers(0, 1 << n, 300, dtype=np.uint64)
    z[:4] = [1 << (n - 1), (1 << n) - 1, 3 << (n - 2), (1 << 27) | 1]
    assert np.count_nonzero(z >> np.uint64(27)) > 200                      # high bits in most masks
    co = rng.standard_normal(300)
    return z, co * (WEIGHT / (abs(gamma) * float(np.sum(np.abs(co)))))


# ---- the checks, for any n -----------------------------------------------------------------------------------------------
def _check_base_state(c, f, what):
    _prepare(c, f)
    worst = _windows(c, lambda idx: ref.amplitudes(f, idx), what)
    _scalar(c.norm2(), 1.0, f"{what} norm2")
    return worst


def _check_rotations(c, n, bra=None):
    f = _f(n, "psi")
    rots = _rotations(n)
    x, z = _masks(rots)
    th = np.array([r[2] for r in rots])
    pass_of, tiles = plan_pauli_rotations(n, x)
    assert [int(p) for p in pass_of] == [0, 0, 0, 1] and int(tiles[0]) >> (n - 1) == 1 and int(tiles[1]) == 0   # tile with the top bit, wide
    _prepare(c, f)
    c.profile_begin()
    passes = c.apply_pauli_rotations(x, z, th)
    entry = [e for e in c.profile_end() if e["kernel"].startswith("k_rot")]
    assert passes == c.last_rotation_passes == len(tiles)
    assert len(entry) == 1 and entry[0]["launches"] == entry[0]["streaming_launches"] == passes, entry   # the non-temporal forms
    ps = [(1.0, f)]
    for xt, zt, t in rots:
        ps = ref.rotate(ps, xt, zt, t)
    assert len(ps) == 16
    _windows(c, lambda idx: ref.sum_amplitudes(ps, idx), f"n={n} four rotations")
    _scalar(c.norm2(), 1.0, "norm2 after the rotations")
    if bra is not None:
        want = ref.inner([(1.0, _f(n, "phi"))], ps)
        assert abs(want) > 0.01
        _scalar(c.overlap(bra), want, "<phi|psi'>")
    sx, sz = _masks(_six_strings(n))
    got = c.expectation_pauli(sx, sz)
    want = np.array([ref.expectation(ps, int(a), int(b)) for a, b in zip(sx, sz)])
    _scalar(float(np.max(np.abs(got - want))), 0.0, "six expectation values, the largest deviation")
    assert float(np.max(np.abs(want))) > 0.01


def _check_diagonal(c, n, bra=None):
    f = _f(n, "psi")
    top, sub = 1 << (n - 1), 1 << (n - 2)
    z4 = np.array([top, top | (1 << 27) | 1, (1 << 12) | (1 << 3), sub | (1 << 20) | (1 << 5) | (1 << 1)], dtype=np.uint64)
    c4, gamma4 = np.array([0.8, -0.5, 0.3, 0.6]), 0.9
    _prepare(c, f)
    c.apply_diagonal_phase(z4, c4, gamma4)
    ps = [(1.0, f)]
    for zt, ct in zip(z4, c4):
        ps = ref.rotate(ps, 0, int(zt), gamma4 * ct)                        # exp(-i gamma c Z..Z), a rotation with x = 0
    _windows(c, lambda idx: ref.sum_amplitudes(ps, idx), f"n={n} four diagonal terms")
    if bra is not None:
        _scalar(c.overlap(bra), ref.inner([(1.0, _f(n, "phi"))], ps), "<phi|exp(-i gamma D)|psi>")
    gamma = -1.3
    z, co = _long_diagonal(n, 290 + n, gamma)
    s = float(np.sum(np.abs(co)))
    _prepare(c, f)
    before = _window_bytes(c)
    got, want = c.diagonal_moments(z, co), ref.diag_moments(f, z, co)
    _scalar(got[0], want[0], "moments of 300 terms: sum p")
    _scalar(got[1], want[1], "sum p E / sum|c|", s)
    _scalar(got[2], want[2], "sum p E^2 / (sum|c|)^2", s * s)
    assert _window_bytes(c) == before                                        # the moments only read
    c.apply_diagonal_phase(z, co, gamma)
    _windows(c, lambda idx: ref.amplitudes(f, idx) * ref.diag_phase(idx, z, co, gamma), f"n={n} phase of 300 terms")
    _scalar(c.norm2(), 1.0, "norm2 after the phase")


def _check_rdm(c, n):
    f = _f(n, "psi")
    top, sub = 1 << (n - 1), 1 << (n - 2)
    _prepare(c, f)
    x, z = top | (1 << 7) | 1, sub | (1 << 2)                                  # entangles bits 0, 2, 7, n - 2, n - 1
    assert c.apply_pauli_rotations([x], [z], [0.6]) == 1
    ps = ref.rotate([(1.0, f)], x, z, 0.6)
    for qubits in ([n - 1], [n - 1, 0, 11], [2, n - 1, 0, 20, n - 2, 11]):
        got, want = c.reduced_density_matrix(qubits), ref.rdm(ps, qubits)
        _scalar(float(np.max(np.abs(got - want))), 0.0, f"n={n} rdm of {qubits}, the largest deviation")
        assert abs(np.trace(want @ want).real - 1.0) > 1e-3                   # mixed: the qubits are entangled with the rest


def _check_sampling(c, n, beyond):
    f = _f(n, "psi")
    _prepare(c, f)
    r = np.concatenate([sampling.draw(4096, seed=n), [0.0, np.nextafter(1.0, 0.0), 0.5]])
    idx = c.sample(r)
    assert idx.dtype == np.uint64 and c.last_sample_passes == 2
    bad = ref.shot_failures(f, r, idx)
    print(f"  n={n}: {r.size} shots, {bad.size} miss the criterion; {np.count_nonzero(idx >= np.uint64(beyond))} indices >= {beyond}")
    assert bad.size == 0, (bad[:5], idx[bad[:5]], r[bad[:5]])
    _scalar(c.last_sample_total, 1.0, "last_sample_total")
    assert np.any(idx >= np.uint64(beyond))
    assert idx.tobytes() == c.sample(r).tobytes()                             # two calls give the same bits


# ---- n = 29 --------------------------------------------------------------------------------------------------------------
def test_29q_base_states(chunks):
    with _Timer("n=29 base states"):
        _check_base_state(chunks[0], _f(N, "psi"), "psi")
        _check_base_state(chunks[1], _f(N, "phi"), "phi")
        want = ref.inner([(1.0, _f(N, "phi"))], [(1.0, _f(N, "psi"))])
        assert abs(want) > 0.5                                                # <phi|psi> is O(1)
        _scalar(chunks[0].overlap(chunks[1]), want, "<phi|psi>")


def test_29q_rotations(chunks):
    with _Timer("n=29 rotations"):
        _prepare(chunks[1], _f(N, "phi"))
        _check_rotations(chunks[0], N, bra=chunks[1])


def test_29q_apply_pauli_sum(chunks):
    src, _, dst = chunks
    f = _f(N, "psi")
    with _Timer("n=29 apply_pauli_sum"):
        x, z = _masks(_sum_terms(N))
        co = np.random.default_rng(291).standard_normal(len(x))
        co /= np.sum(np.abs(co))
        tiles = [int(t) for t in plan_expectation(N, x)[1]]
        assert len(tiles) == 2 and tiles[0] >> (N - 1) == 1 and tiles[1] == 0  # one writing tile pass, one accumulating wide pass
        _prepare(src, f)
        dst.init_random(5)
        before = _window_bytes(src)
        assert dst.apply_pauli_sum(src, x, z, co) == dst.last_pauli_sum_passes == 2
        h = ref.apply_sum([(1.0, f)], [int(v) for v in x], [int(v) for v in z], co)
        _windows(dst, lambda idx: ref.sum_amplitudes(h, idx), "H psi, eight terms")
        want = ref.inner(h, h).real
        assert want > 0.01
        _scalar(dst.norm2(), want, "|H psi|^2")
        assert _window_bytes(src) == before                                    # src is only read


def test_29q_overlap_pauli(chunks):
    ket, bra, _ = chunks
    f, g = _f(N, "psi"), _f(N, "phi")
    full = (1 << N) - 1
    with _Timer("n=29 overlap_pauli"):
        x, z = _masks(_sum_terms(N) + [(full, 0), (full, full), ((1 << (N - 1)) | 1, 1), (0, full)])
        assert len(x) == 12
        tiles = [int(t) for t in plan_expectation(N, x)[1]]
        assert tiles.count(0) == 3 and len(tiles) > 3                          # tile and wide passes
        _prepare(ket, f)
        _prepare(bra, g)
        got = ket.overlap_pauli(bra, x, z)
        assert ket.last_overlap_passes == len(tiles)
        want = np.array([ref.inner([(1.0, g)], [(1.0, ref.pauli_on(f, int(a), int(b)))]) for a, b in zip(x, z)])
        _scalar(float(np.max(np.abs(got - want))), 0.0, "<phi|P_t|psi> of twelve strings, the largest deviation")
        assert np.count_nonzero(np.abs(want) > 0.01) >= 6
        own = ket.overlap_pauli(ket, x, z)
        _scalar(float(np.max(np.abs(own - ket.expectation_pauli(x, z)))), 0.0, "<psi|P_t|psi> against expectation_pauli")
        _scalar(float(np.max(np.abs(own.real - [ref.expectation([(1.0, f)], int(a), int(b)) for a, b in zip(x, z)]))), 0.0,
                "<psi|P_t|psi> against the closed form")


def test_29q_lincomb(chunks):
    s0, s1, dst = chunks
    psi, phi, chi, omega = (_f(N, w) for w in ("psi", "phi", "chi", "omega"))
    with _Timer("n=29 lincomb"):
        extra = DeviceChunk.empty(N)                                           # a bra that is no source
        try:
            for c, f in ((s0, psi), (s1, phi), (dst, chi), (extra, omega)):
                _prepare(c, f)
            dc, co = 0.3 - 0.2j, [0.25j, -0.35]                                # sum |a| < 1
            dst.profile_begin()
            dots, norm2 = dst.lincomb(dc, [s0, s1], co, [s1, extra], True)
            entry = [e for e in dst.profile_end() if e["kernel"].startswith("k_lincomb")]
            assert len(entry) == 1 and entry[0]["launches"] == entry[0]["streaming_launches"] == 1, entry
            want = [(dc, chi), (co[0], psi), (co[1], phi)]
            _windows(dst, lambda idx: ref.sum_amplitudes(want, idx), "a_d dst + a_0 psi + a_1 phi")
            _scalar(dots[0], ref.inner([(1.0, phi)], want), "<phi|dst>, the bra on a source")
            _scalar(dots[1], ref.inner([(1.0, omega)], want), "<omega|dst>")
            _scalar(norm2, ref.inner(want, want).real, "|dst|^2")
            assert abs(ref.inner([(1.0, phi)], want)) > 0.01
            # the form without reductions: one workgroup per block, 2^19 of them
            dc2, c2 = -0.4 + 0.3j, 0.45j
            dots2, none = dst.lincomb(dc2, [s0], [c2])
            assert dots2.size == 0 and none is None
            want2 = [(dc2 * a, f) for a, f in want] + [(c2, psi)]
            _windows(dst, lambda idx: ref.sum_amplitudes(want2, idx), "a_d dst + a_0 psi, nothing reduced")
            _scalar(dst.norm2(), ref.inner(want2, want2).real, "|dst|^2 by norm2")
        finally:
            extra.close()


def test_29q_diagonal(chunks):
    with _Timer("n=29 diagonal"):
        _prepare(chunks[1], _f(N, "phi"))
        _check_diagonal(chunks[0], N, bra=chunks[1])


def test_29q_rdm(chunks):
    with _Timer("n=29 rdm"):
        _check_rdm(chunks[0], N)


def test_29q_sampling(chunks):
    with _Timer("n=29 sampling"):
        _check_sampling(chunks[0], N, 1 << 28)


# ---- n = 32: the in-place and read-only calls on one chunk ---------------------------------------------------------------
def test_32q_base_state(big):
    with _Timer("n=32 base state"):
        _check_base_state(big, _f(BIG, "psi"), "psi")


def test_32q_rotations_and_expectation(big):
    with _Timer("n=32 rotations"):
        _check_rotations(big, BIG)


def test_32q_diagonal(big):
    with _Timer("n=32 diagonal"):
        _check_diagonal(big, BIG)


def test_32q_rdm(big):
    with _Timer("n=32 rdm"):
        _check_rdm(big, BIG)


def test_32q_sampling(big):
    with _Timer("n=32 sampling"):
        _check_sampling(big, BIG, 1 << 31)
