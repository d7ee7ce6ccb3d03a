"""qsim_apply_diagonal_phase and qsim_diagonal_moments on an MI355X against the direct sum of tests/diagonal_reference.

Bounds.  The phase is held to the project's 1e-12 absolute on unit-norm states, every list scaled so that |gamma| sum|c_t|
= 32.  The derived error of the phase is about (tb + log2 T) eps * 32 ~ 1e-13: E is a sum of T terms of total weight
sum|c| followed by tb = 11 add/sub stages, each adding one rounding relative to sum|c|, and the angle gamma E carries that
times |gamma|.  A numpy model of the tiled algorithm against the direct sum (n = 5 / 11 / 13 / 14, T = 40 ... 2048) gave a
phase error <= 1.1e-14 and an amplitude error <= 1.1e-15, so the reference stays three orders inside the bound.  Moments:
1e-12 relative to sum|c_t| for the mean and to (sum|c_t|)^2 for the second moment (unit-norm states)."""
import numpy as np
import pytest

from quantum_simulations_amd import _lib, diagonal, evolution
from quantum_simulations_amd import circuits as gen
from quantum_simulations_amd.circuit.staging import permute_state
from quantum_simulations_amd.kernel.device import DeviceChunk
from quantum_simulations_amd.observable import PauliSum
from tests import diagonal_reference as ref
from tests.rotation_reference import rotate_list

pytestmark = pytest.mark.gpu

ATOL = 1e-12
WEIGHT = 32.0            # |gamma| sum |c_t| of every compared list
KERNEL = "k_diag diagonal Pauli sum"


def _rand_state(n, seed):
    rng = np.random.default_rng(seed)
    psi = rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)
    return psi / np.linalg.norm(psi)


def _subset(rng, bits, w):
    m = 0
    for b in rng.choice(bits, size=w, replace=False):
        m |= 1 << int(b)
    return m


def _lists(n, seed):
    """{name: z masks}: the lists of one chunk size."""
    rng = np.random.default_rng(seed)
    full = (1 << n) - 1
    lo_bits, hi_bits = list(range(min(n, 11))), list(range(11, n))
    out = {"singles": [1 << q for q in range(n)],
           "pairs": [(1 << a) | (1 << b) for a in range(n) for b in range(a + 1, n)] or [1],
           "weights": [_subset(rng, n, 1 + i % n) for i in range(64)],
           "identity": [0],
           "full": [full],
           "low": [_subset(rng, lo_bits, int(rng.integers(1, len(lo_bits) + 1))) for _ in range(30)]}
    if hi_bits:
        out["high"] = [_subset(rng, hi_bits, int(rng.integers(1, len(hi_bits) + 1))) for _ in range(20)]
    # 300 terms on 7 distinct inner parts: segments of about 43 and, with the repeats below, of more than 64 terms (pieces)
    inner = [_subset(rng, lo_bits, int(rng.integers(1, len(lo_bits) + 1))) for _ in range(6)] + [0]
    pick = rng.integers(0, 7, size=300)
    pick[:150] = np.where(pick[:150] < 2, pick[:150], 0)              # inner[0] gets about 110 terms: two pieces
    out["long_segments"] = [inner[int(p)] | (_subset(rng, hi_bits, int(rng.integers(0, len(hi_bits) + 1))) if hi_bits else 0) for p in pick]
    dup = [_subset(rng, n, 1 + i % n) for i in range(5)]
    out["duplicates"] = dup + dup[::-1] + dup[:2] + [0, 0]
    out["zero_coefficients"] = [_subset(rng, n, 1 + i % n) for i in range(12)]
    return {k: np.array(v, dtype=np.uint64) for k, v in out.items()}


def _coeffs(rng, name, count, gamma):
    c = rng.standard_normal(count)
    if name == "zero_coefficients":
        c[::3] = 0.0
    return c * (WEIGHT / (abs(gamma) * float(np.sum(np.abs(c)))))


def _check_phase_and_moments(c, psi, z, co, gamma, what):
    c.upload(psi)
    c.apply_diagonal_phase(z, co, gamma)
    got = c.download()
    err = float(np.max(np.abs(got - ref.phase(psi, z, co, gamma))))
    c.upload(psi)
    n2, m1, m2 = c.diagonal_moments(z, co)
    w2, w1, ww = ref.moments(psi, z, co)
    s = float(np.sum(np.abs(co)))
    e0, e1, e2 = abs(n2 - w2), abs(m1 - w1) / s, abs(m2 - ww) / (s * s)
    print(f"{what}: {z.size} terms, phase max |got - want| = {err:.3e} (bound {ATOL:g}); moments: norm {e0:.2e}, "
          f"mean / sum|c| {e1:.2e}, second / (sum|c|)^2 {e2:.2e} (bound {ATOL:g})")
    assert err < ATOL, (what, err)
    assert e0 < ATOL and e1 < ATOL and e2 < ATOL, (what, e0, e1, e2)
    assert np.array_equal(c.download(), psi), what                       # the moments read only


@pytest.mark.parametrize("n", list(range(1, 15)))
def test_against_the_reference(n):
    psi = _rand_state(n, n)
    rng = np.random.default_rng(700 + n)
    c = DeviceChunk.empty(n)
    try:
        for name, z in _lists(n, 300 + n).items():
            gamma = float(rng.choice([0.7, -1.3, 2.9]))
            _check_phase_and_moments(c, psi, z, _coeffs(rng, name, z.size, gamma), gamma, f"n={n} {name}")
        z = _lists(n, 300 + n)["weights"]
        c.upload(psi)
        c.apply_diagonal_phase(z, _coeffs(rng, "weights", z.size, 1.0), 0.0)
        assert c.download().tobytes() == psi.tobytes()                    # gamma = 0: the same bits
        c.profile_begin()
        c.apply_diagonal_phase([], [], 0.5)                               # no terms: nothing is launched
        assert c.profile_end() == []
        assert c.download().tobytes() == psi.tobytes()
        n2, m1, m2 = c.diagonal_moments([], [])
        assert abs(n2 - 1.0) < 1e-13 and m1 == 0.0 and m2 == 0.0
    finally:
        c.close()


def test_against_the_rotation_path():
    """The same Z-only list through qsim_apply_pauli_rotations (theta_t = gamma c_t) on a second chunk."""
    n, T = 13, 128
    rng = np.random.default_rng(71)
    psi = _rand_state(n, 70)
    z = np.array([_subset(rng, n, 1 + i % n) for i in range(T)], dtype=np.uint64)
    gamma = -0.8
    co = _coeffs(rng, "", T, gamma)
    a, b = DeviceChunk.from_numpy(psi), DeviceChunk.from_numpy(psi)
    try:
        a.apply_diagonal_phase(z, co, gamma)
        b.apply_pauli_rotations(np.zeros(T, dtype=np.uint64), z, gamma * co)
        got, other = a.download(), b.download()
        err = float(np.max(np.abs(got - other)))
        print(f"diagonal pass against {T} Z rotations: max |difference| = {err:.3e} (bound {ATOL:g})")
        assert err < ATOL
        assert float(np.max(np.abs(got - psi))) > 1e-3
    finally:
        a.close()
        b.close()


def test_inverse_norm_and_repeatability():
    n = 13
    rng = np.random.default_rng(72)
    psi = _rand_state(n, 73)
    lists = _lists(n, 74)
    z = np.concatenate([lists["weights"], lists["high"], lists["long_segments"], lists["duplicates"]])
    gamma = 1.7
    co = _coeffs(rng, "", z.size, gamma)
    c = DeviceChunk.from_numpy(psi)
    try:
        c.apply_diagonal_phase(z, co, gamma)
        first = c.download()
        assert abs(c.norm2() - 1.0) < 1e-13
        assert float(np.max(np.abs(first - psi))) > 1e-3
        c.apply_diagonal_phase(z, co, -gamma)
        back = float(np.max(np.abs(c.download() - psi)))
        print(f"+gamma then -gamma over {z.size} terms: max |after - before| = {back:.3e} (bound {ATOL:g})")
        assert back < ATOL
        c.upload(psi)
        c.apply_diagonal_phase(z, co, gamma)
        assert c.download().tobytes() == first.tobytes()                  # the same bits from the same start
        m_a, m_b = c.diagonal_moments(z, co), c.diagonal_moments(z, co)
        assert np.array(m_a).tobytes() == np.array(m_b).tobytes()
    finally:
        c.close()


def test_term_limit():
    n, T = 12, 16384
    rng = np.random.default_rng(75)
    psi = _rand_state(n, 76)
    z = rng.integers(0, 1 << n, size=T + 1, dtype=np.uint64)
    z[:200] = np.uint64(1 << 11)                                          # one segment of 200 + terms: four pieces
    gamma = 0.9
    co = np.append(_coeffs(rng, "", T, gamma), 0.25)
    c = DeviceChunk.empty(n)
    try:
        _check_phase_and_moments(c, psi, z[:T], co[:T], gamma, f"n={n} {T} terms")
        c.upload(psi)
        lib = _lib.load()
        out = np.zeros(3)
        assert lib.qsim_apply_diagonal_phase(c._h, T + 1, _lib.ptr(z), _lib.ptr(co), gamma) == _lib.QSIM_ERR_INVALID
        assert lib.qsim_diagonal_moments(c._h, T + 1, _lib.ptr(z), _lib.ptr(co), _lib.ptr(out)) == _lib.QSIM_ERR_INVALID
        with pytest.raises(ValueError, match="16384"):
            c.apply_diagonal_phase(z, co, gamma)
        assert c.download().tobytes() == psi.tobytes()
    finally:
        c.close()


def test_grid_stride_loop_at_22_qubits():
    """2^22 amplitudes: 2048 tiles, two per workgroup under the cap of 1024 workgroups."""
    n = 22
    rng = np.random.default_rng(77)
    psi = _rand_state(n, 78)
    z = [1 << 21, 1 << 20, 3 << 20, (1 << 21) | 5, (1 << 20) | (1 << 10), (1 << n) - 1, 0, 1, 0x7FF, (1 << 21) | (1 << 11)]
    z += [_subset(rng, n, int(rng.integers(1, n + 1))) for _ in range(30)]
    z = np.array(z, dtype=np.uint64)
    assert z.size == 40
    gamma = -1.1
    _c = DeviceChunk.empty(n)
    try:
        _check_phase_and_moments(_c, psi, z, _coeffs(rng, "", z.size, gamma), gamma, "n=22")
    finally:
        _c.close()


def test_streaming_instantiation():
    """A 12-qubit view inside a 2^25 allocation (512 MiB, more than the 256 MiB Infinity Cache): the non-temporal forms of
    k_diag_tile.  Only the view and the 2^12 amplitudes on either side are uploaded and downloaded."""
    n, w = 12, 1 << 12
    off = 1234 * w
    window = _rand_state(n + 2, 79)[:3 * w]                     # left guard | view | right guard
    psi = window[w:2 * w]
    rng = np.random.default_rng(80)
    lists = _lists(n, 81)
    z = np.concatenate([lists["weights"], lists["high"], lists["long_segments"]])
    gamma = 0.6
    co = _coeffs(rng, "", z.size, gamma)
    parent = DeviceChunk.empty(25)
    view = parent.view(off, n)
    try:
        parent.upload(window, offset=off - w)
        view.profile_begin()
        n2, m1, m2 = view.diagonal_moments(z, co)
        entry = [e for e in view.profile_end() if e["kernel"] == KERNEL]
        assert len(entry) == 1 and entry[0]["launches"] == entry[0]["streaming_launches"] == 1, entry
        assert entry[0]["algorithmic_bytes"] == entry[0]["hbm_bytes"] == 16.0 * w
        want = ref.moments(psi, z, co)
        s = float(np.sum(np.abs(co)))
        assert abs(n2 - want[0]) < ATOL and abs(m1 - want[1]) < ATOL * s and abs(m2 - want[2]) < ATOL * s * s
        view.profile_begin()
        view.apply_diagonal_phase(z, co, gamma)
        entry = [e for e in view.profile_end() if e["kernel"] == KERNEL]
        assert len(entry) == 1 and entry[0]["launches"] == entry[0]["streaming_launches"] == 1, entry
        assert entry[0]["algorithmic_bytes"] == entry[0]["hbm_bytes"] == 32.0 * w
        got = parent.download(off - w, 3 * w)
        assert float(np.max(np.abs(got[w:2 * w] - ref.phase(psi, z, co, gamma)))) < ATOL
        assert got[:w].tobytes() == window[:w].tobytes() and got[2 * w:].tobytes() == window[2 * w:].tobytes()
    finally:
        view.close()
        parent.close()


def test_errors():
    from tests.test_gpu_kernels import _random_ops
    k = 14
    psi = _rand_state(k, 82)
    lib = _lib.load()
    c, buf = DeviceChunk.from_numpy(psi), DeviceChunk.empty(k)
    try:
        def phase(z, co, gamma=0.3, n=None, handle=c._h):
            zs = None if z is None else np.array(z, dtype=np.uint64)
            cs = None if co is None else np.array(co, dtype=np.float64)
            return lib.qsim_apply_diagonal_phase(handle, 2 if n is None else n, _lib.ptr(zs), _lib.ptr(cs), gamma)

        def moments(z, co, n=None, handle=c._h, out=True):
            zs = None if z is None else np.array(z, dtype=np.uint64)
            cs = None if co is None else np.array(co, dtype=np.float64)
            res = np.zeros(3)
            return lib.qsim_diagonal_moments(handle, 2 if n is None else n, _lib.ptr(zs), _lib.ptr(cs), _lib.ptr(res) if out else None)

        ok = ([1, 6], [0.1, 0.2])
        for call in (phase, moments):
            for zm in (1 << k, 1 << (k + 1), 1 << 63):
                assert call([1, zm], ok[1]) == _lib.QSIM_ERR_NONLOCAL
            assert b"index bit" in lib.qsim_last_error() and b"log2(chunk_size)=14" in lib.qsim_last_error()
            for bad in (float("nan"), float("inf"), -float("inf")):
                assert call(ok[0], [0.1, bad]) == _lib.QSIM_ERR_INVALID
            assert call(None, ok[1]) == _lib.QSIM_ERR_INVALID
            assert call(ok[0], None) == _lib.QSIM_ERR_INVALID
            assert call(*ok, handle=None) == _lib.QSIM_ERR_INVALID
            assert call(*ok, n=-1) == _lib.QSIM_ERR_INVALID
            assert call(None, None, n=0) == _lib.QSIM_OK
        for bad in (float("nan"), float("inf"), -float("inf")):
            assert phase(*ok, gamma=bad) == _lib.QSIM_ERR_INVALID
        assert moments(*ok, out=False) == _lib.QSIM_ERR_INVALID
        with pytest.raises(NotImplementedError):
            c.apply_diagonal_phase([1 << k], [0.1], 0.2)
        with pytest.raises(NotImplementedError):
            c.diagonal_moments([1 << k], [0.1])
        with pytest.raises(ValueError):
            c.apply_diagonal_phase([1], [float("nan")], 0.2)
        with pytest.raises(ValueError):
            c.apply_diagonal_phase([1, 2], [0.1], 0.2)
        with pytest.raises(ValueError):
            c.diagonal_moments([1, 2], [0.1])
        assert c.download().tobytes() == psi.tobytes()          # a refused call changes nothing
        # a split qsim_apply_ops_io has left pieces pending on the chunk: refused like a plain op list
        c.apply_ops_io(_random_ops(k, 10, 1), dst=(buf, [5], None, -1), parts=-2)
        assert c.pending_parts()
        with pytest.raises(ValueError, match="pending"):
            c.apply_diagonal_phase(*ok, 0.3)
        with pytest.raises(ValueError, match="pending"):
            c.diagonal_moments(*ok)
        for j in range(len(c.pending_parts())):
            c.store_part(j)
        assert phase(*ok) == _lib.QSIM_OK and moments(*ok) == _lib.QSIM_OK
    finally:
        c.close()
        buf.close()


# ---- the engine and the runner -------------------------------------------------------------------------------------------
def _ring_maxcut(n):
    return PauliSum([(0.5, {q: "Z", (q + 1) % n: "Z"}) for q in range(n)] + [(-0.5 * n, {})], n_qubits=n)


def _dense(obs):
    mats = {"I": np.eye(2), "X": np.array([[0, 1], [1, 0]]), "Y": np.array([[0, -1j], [1j, 0]]), "Z": np.diag([1.0, -1.0])}
    H = np.zeros((1 << obs.n_qubits,) * 2, dtype=np.complex128)
    for x, z, c in zip(obs.x, obs.z, obs.coeffs):
        M = np.eye(1, dtype=np.complex128)
        for q in range(obs.n_qubits):
            bx, bz = (x >> q) & 1, (z >> q) & 1
            M = np.kron(mats["Y" if bx and bz else "X" if bx else "Z" if bz else "I"], M)
        H += c * M
    return H


def _qaoa_dense(psi, cost, gammas, betas):
    from scipy.linalg import expm
    n = cost.n_qubits
    C_, B_ = _dense(cost), _dense(PauliSum([(1.0, {q: "X"}) for q in range(n)], n_qubits=n))
    for g, b in zip(gammas, betas):
        psi = expm(-1j * b * B_) @ (expm(-1j * g * C_) @ psi)
    return psi


def _qaoa_reference(psi, cost, gammas, betas):
    n = cost.n_qubits
    z, co = diagonal.diagonal_part(cost)
    for g, b in zip(gammas, betas):
        psi = rotate_list(ref.phase(psi, z, co, g), [1 << q for q in range(n)], [0] * n, [b] * n)
    return psi


GAMMAS, BETAS = [0.4, -0.9, 1.3], [0.7, 0.2, -0.5]


def test_engine_qaoa_moments_and_fused_evolution():
    from quantum_simulations_amd.runner.engine import SingleGpuEngine
    n = 12
    eng = SingleGpuEngine(n, layout="search")
    try:
        eng.init_zero_state()
        eng.execute(eng.plan(gen.random_1q_cx_circuit(n, depth=6, seed=9), repeats=8))
        l2p = [int(p) for p in np.random.default_rng(3).permutation(n)]
        eng._adopt_layout(l2p)
        assert eng.l2p == l2p and l2p != list(range(n))
        cost = _ring_maxcut(n)
        psi = eng.state_vector()
        passes = eng.qaoa(cost, GAMMAS, BETAS)
        assert passes >= 2 * len(GAMMAS) and eng.l2p == l2p and not eng._zero        # the state did not move
        got = eng.state_vector()
        assert float(np.max(np.abs(got - _qaoa_reference(psi, cost, GAMMAS, BETAS)))) < 1e-11
        mean, var = eng.diagonal_moments(cost)
        assert abs(mean - eng.expectation(cost)) < 1e-11 and abs(var - eng.variance(cost)) < 1e-11
        assert eng.apply_diagonal_phase(cost, 0.45) == 1
        z, co = diagonal.diagonal_part(cost)
        assert float(np.max(np.abs(eng.state_vector() - ref.phase(got, z, co, 0.45)))) < 1e-11
    finally:
        eng.close()
    # against dense matrices
    n = 6
    eng = SingleGpuEngine(n, layout="identity")
    try:
        eng.init_random_state(5)
        psi = eng.state_vector()
        cost = _ring_maxcut(n)
        eng.qaoa(cost, GAMMAS, BETAS)
        err = float(np.max(np.abs(eng.state_vector() - _qaoa_dense(psi, cost, GAMMAS, BETAS))))
        print(f"engine qaoa, n = 6, 3 layers against dense expm: {err:.3e} (bound 1e-11)")
        assert err < 1e-11
    finally:
        eng.close()


def test_engine_evolve_fuse_diagonal():
    """The transverse-field Ising chain at n = 13, second order: where two steps meet, the 12 ZZ bonds that end one and
    the 12 that begin the next are one run of 24 Z strings, which becomes one diagonal pass."""
    from quantum_simulations_amd.runner.engine import SingleGpuEngine
    n = 13
    assert evolution.DIAGONAL_MIN_RUN <= 2 * (n - 1)
    H = PauliSum([(1.0, {q: "Z", q + 1: "Z"}) for q in range(n - 1)] + [(0.7, {q: "X"}) for q in range(n)], n_qubits=n)
    a, b = SingleGpuEngine(n, layout="identity"), SingleGpuEngine(n, layout="identity")
    try:
        a.init_random_state(6)
        b.init_random_state(6)
        plain = a.evolve(H, 0.3, steps=3, order=2)
        fused = b.evolve(H, 0.3, steps=3, order=2, fuse_diagonal=True)
        assert plain >= 1 and fused != plain, (plain, fused)      # the two runs of 24 are passes of their own now
        err = float(np.max(np.abs(a.state_vector() - b.state_vector())))
        print(f"evolve with and without fuse_diagonal: max |difference| = {err:.3e} (bound {ATOL:g})")
        assert err < ATOL
    finally:
        a.close()
        b.close()


def test_single_node_qaoa():
    from quantum_simulations_amd.runner import single_node
    n = 12
    buf = single_node.run(gen.random_1q_cx_circuit(n, depth=8, seed=5), chunk_size=1 << 9, use_fusion=True, use_staging=True)
    try:
        l2p = getattr(buf, "log_to_phys", None) or None
        assert l2p and l2p != list(range(n))
        psi = permute_state(buf.state.download(), l2p)
        cost = _ring_maxcut(n)
        assert single_node.qaoa(buf, cost, GAMMAS, BETAS) >= 2 * len(GAMMAS)
        got = permute_state(buf.state.download(), l2p)
        assert float(np.max(np.abs(got - _qaoa_reference(psi, cost, GAMMAS, BETAS)))) < 1e-11
        mean, var = single_node.diagonal_moments(buf, cost)
        assert abs(mean - single_node.expectation(buf, cost)) < 1e-11 and abs(var - single_node.variance(buf, cost)) < 1e-11
        assert single_node.apply_diagonal_phase(buf, cost, -0.2) == 1
        z, co = diagonal.diagonal_part(cost)
        assert float(np.max(np.abs(permute_state(buf.state.download(), l2p) - ref.phase(got, z, co, -0.2)))) < 1e-11
    finally:
        buf.close()
    n = 6
    buf = single_node.run(gen.random_1q_cx_circuit(n, depth=4, seed=2), chunk_size=1 << n, use_fusion=True, use_staging=False)
    try:
        l2p = getattr(buf, "log_to_phys", None) or None
        logical = (lambda v: v) if l2p is None else (lambda v: permute_state(v, l2p))
        psi = logical(buf.state.download())
        cost = _ring_maxcut(n)
        single_node.qaoa(buf, cost, GAMMAS, BETAS)
        err = float(np.max(np.abs(logical(buf.state.download()) - _qaoa_dense(psi, cost, GAMMAS, BETAS))))
        print(f"single_node qaoa, n = 6, 3 layers against dense expm: {err:.3e} (bound 1e-11)")
        assert err < 1e-11
    finally:
        buf.close()
