"""qsim_apply_pauli_sum (dst = sum_t c_t P_t src) and qsim_overlap_pauli (<bra|P_t|ket>) on an MI355X against the host
references of tests/twostate_reference.py, and the host module `hamiltonian` (variance, adjoint gradients) through the
engine and the runner.  Coefficients are normalised to sum |c_t| = 1 and states to unit norm, so the project's absolute
bound of 1e-12 (tests/test_gpu_expectation.py, tests/test_gpu_pauli_rotation.py) is meaningful: an amplitude of H psi is
a sum of at most 4096 products of size <= |c_t|, a matrix element a sum of 2^n products of total size <= 1, each rounded
to a few 1e-16.  Gradients over at most 32 rotations use 1e-11 (two rotations per parameter on both chunks before the
overlap is read)."""
import ctypes as C

import numpy as np
import pytest

from quantum_simulations_amd import _lib
from quantum_simulations_amd import circuits as gen
from quantum_simulations_amd.circuit.staging import permute_state
from quantum_simulations_amd.kernel.device import DeviceChunk, plan_expectation
from quantum_simulations_amd.observable import PauliSum
from tests.pauli_reference import apply_pauli
from tests.test_gpu_pauli_rotation import _lists, _rand_state
from tests.twostate_reference import apply_sum, gradient_forward, matrix_elements

pytestmark = pytest.mark.gpu

ATOL = 1e-12
GRAD_ATOL = 1e-11


def _arrays(pairs, rng):
    x = np.array([p[0] for p in pairs], dtype=np.uint64)
    z = np.array([p[1] for p in pairs], dtype=np.uint64)
    co = rng.uniform(-1.0, 1.0, len(pairs))
    return x, z, co / np.sum(np.abs(co))


def _families(n, seed):
    """The term families of tests/test_gpu_pauli_rotation._lists, and for n >= 12 `wide_only`: no term fits a tile, so
    the FIRST (writing) pass is a wide one and the later wide passes accumulate; in `wide` the wide passes come after the
    tile passes (the order of plan_expectation), so there they all accumulate."""
    out = dict(_lists(n, seed))
    if n >= 12:
        full = (1 << n) - 1
        out["wide_only"] = [(full, 0), (full, full), (full ^ 0b111, 0b101), (full & ~1, (1 << (n - 1)) | 1)]
    return out


def _n_passes(k, x):
    return len(plan_expectation(k, x)[1])


# ---- qsim_apply_pauli_sum ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", list(range(1, 15)))
def test_apply_pauli_sum_against_the_reference(n):
    psi = _rand_state(n, n)
    rng = np.random.default_rng(600 + n)
    src, dst = DeviceChunk.from_numpy(psi), DeviceChunk.empty(n)
    try:
        made = {}
        for name, pairs in _families(n, 100 + n).items():
            x, z, co = _arrays(pairs, rng)
            dst.init_random(7 + n)                                  # what dst held must not matter
            passes = dst.apply_pauli_sum(src, x, z, co)
            err = float(np.max(np.abs(dst.download() - apply_sum(psi, x, z, co))))
            print(f"n={n} {name}: {len(pairs)} terms in {passes} passes, max |got - want| = {err:.3e} (bound {ATOL:g})")
            assert err < ATOL, (name, err)
            assert passes == dst.last_pauli_sum_passes == _n_passes(n, x), name
            made[name] = (passes, [int(t) for t in plan_expectation(n, x)[1]])
        assert src.download().tobytes() == psi.tobytes()           # src is only read
        if n >= 12:
            assert made["breaks"][0] >= 3, made                     # a writing pass and accumulating tile passes
            tiles = made["wide"][1]
            assert tiles[0] != 0 and tiles.count(0) >= 1, made      # wide passes after tile passes: accumulating
            assert made["wide_only"][1] == [0] * 4, made            # a wide pass that writes, three that accumulate
        else:
            assert {p for p, _ in made.values()} == {1}, made       # the whole chunk is one tile
    finally:
        src.close()
        dst.close()


def test_all_4096_strings_on_6_qubits():
    n = 6
    psi, phi = _rand_state(n, 60), _rand_state(n, 61)
    pairs = [(x, z) for x in range(64) for z in range(64)]
    x, z, co = _arrays(pairs, np.random.default_rng(62))
    src, dst, bra = DeviceChunk.from_numpy(psi), DeviceChunk.empty(n), DeviceChunk.from_numpy(phi)
    try:
        dst.init_random(63)
        assert dst.apply_pauli_sum(src, x, z, co) == 4             # 4 passes of 1024 terms
        assert [int(c) for c in np.bincount(plan_expectation(n, x)[0])] == [1024] * 4
        err = float(np.max(np.abs(dst.download() - apply_sum(psi, x, z, co))))
        print(f"4096 strings: H psi max |got - want| = {err:.3e} (bound {ATOL:g})")
        assert err < ATOL
        got = src.overlap_pauli(bra, x, z)
        assert src.last_overlap_passes == 4
        err = float(np.max(np.abs(got - matrix_elements(phi, psi, x, z))))
        print(f"4096 strings: <bra|P|ket> max |got - want| = {err:.3e} (bound {ATOL:g})")
        assert err < ATOL
    finally:
        src.close()
        dst.close()
        bra.close()


def test_special_term_sets():
    n = 13
    psi = _rand_state(n, 64)
    src, dst = DeviceChunk.from_numpy(psi), DeviceChunk.empty(n)
    try:
        dst.init_random(65)
        assert dst.apply_pauli_sum(src, [], [], []) == 0           # no terms: dst := 0
        assert not np.any(dst.download())
        dst.init_random(66)
        assert dst.apply_pauli_sum(src, [0], [0], [1.0]) == 1      # H = I
        assert np.array_equal(dst.download(), psi)
        rng = np.random.default_rng(67)
        full = (1 << n) - 1
        zs = [0, 1, 1 << (n - 1), full, full & ~0x7FF, 0x7FF] + [int(v) for v in rng.integers(0, full + 1, 20)]
        x, z, co = _arrays([(0, m) for m in zs], rng)              # diagonal only
        dst.init_random(68)
        assert dst.apply_pauli_sum(src, x, z, co) == 1
        assert float(np.max(np.abs(dst.download() - apply_sum(psi, x, z, co)))) < ATOL
        assert src.download().tobytes() == psi.tobytes()
    finally:
        src.close()
        dst.close()


# ---- qsim_overlap_pauli -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", list(range(1, 15)))
def test_overlap_pauli_against_the_reference(n):
    psi, phi = _rand_state(n, n), _rand_state(n, 30 + n)
    rng = np.random.default_rng(700 + n)
    ket, bra, work = DeviceChunk.from_numpy(psi), DeviceChunk.from_numpy(phi), DeviceChunk.empty(n)
    try:
        for name, pairs in _families(n, 100 + n).items():
            x, z, co = _arrays(pairs, rng)
            got = ket.overlap_pauli(bra, x, z)
            want = matrix_elements(phi, psi, x, z)
            err = float(np.max(np.abs(got - want)))
            print(f"n={n} {name}: {len(pairs)} terms in {ket.last_overlap_passes} passes, max |got - want| = {err:.3e} (bound {ATOL:g})")
            assert err < ATOL, (name, err)
            assert ket.last_overlap_passes == _n_passes(n, x), name
            assert ket.overlap_pauli(bra, x, z).tobytes() == got.tobytes(), name      # the same bits twice
            back = bra.overlap_pauli(ket, x, z)                      # <a|P|b> = conj(<b|P|a>)
            assert float(np.max(np.abs(got - np.conj(back)))) < ATOL, name
            same = ket.overlap_pauli(ket, x, z)                      # <psi|P|psi>: real
            assert float(np.max(np.abs(same.real - ket.expectation_pauli(x, z)))) < ATOL, name
            assert float(np.max(np.abs(same.imag))) < ATOL, name
            # Re <psi|H psi> = sum_t c_t <psi|P_t|psi>
            work.apply_pauli_sum(ket, x, z, co)
            assert abs(work.overlap(ket).real - float(np.dot(co, ket.expectation_pauli(x, z)))) < ATOL, name
        assert abs(ket.overlap(bra) - np.vdot(phi, psi)) < ATOL
        assert ket.download().tobytes() == psi.tobytes() and bra.download().tobytes() == phi.tobytes()
    finally:
        ket.close()
        bra.close()
        work.close()


# ---- the grid-stride loops --------------------------------------------------------------------------------------------
def test_both_calls_at_22_qubits():
    """2^22 amplitudes: 2048 tiles, two per workgroup of k_psum_tile (1024 workgroups) and four of k_ovl_tile (512)."""
    n = 22
    full = (1 << n) - 1
    psi, phi = _rand_state(n, 70), _rand_state(n, 71)
    pairs = [(1 << 3, 0), (0, 1 << 21), (0x18, 0x10 | 1 << 21), (1 << 21, 1 << 20), (3 << 12, 1 << 12), (full, 5 << 19), (0, 0),
             (0x7F8, full), (1 << 10 | 1 << 20, 1 << 21), (0, full)]
    x, z, co = _arrays(pairs, np.random.default_rng(72))
    tiles = [int(t) for t in plan_expectation(n, x)[1]]
    assert tiles.count(0) == 1 and len(tiles) >= 3
    images = [apply_pauli(psi, int(a), int(b)) for a, b in zip(x, z)]       # P_t psi, once for both references
    want_sum = sum(c * v for c, v in zip(co, images))
    want_me = np.array([np.vdot(phi, v) for v in images])
    src, dst, bra = DeviceChunk.from_numpy(psi), DeviceChunk.empty(n), DeviceChunk.from_numpy(phi)
    try:
        dst.init_random(73)
        assert dst.apply_pauli_sum(src, x, z, co) == len(tiles)
        err = float(np.max(np.abs(dst.download() - want_sum)))
        print(f"n=22: H psi, {len(pairs)} terms in {len(tiles)} passes, max |got - want| = {err:.3e} (bound {ATOL:g})")
        assert err < ATOL
        got = src.overlap_pauli(bra, x, z)
        assert src.last_overlap_passes == len(tiles)
        err = float(np.max(np.abs(got - want_me)))
        print(f"n=22: <bra|P|ket>, max |got - want| = {err:.3e} (bound {ATOL:g})")
        assert err < ATOL
    finally:
        src.close()
        dst.close()
        bra.close()


def test_streaming_instantiations():
    """12-qubit views inside 2^25-amplitude allocations (512 MiB each, more than the 256 MiB Infinity Cache): the
    non-temporal forms of all four kernels, writing and accumulating.  Only the views and the 2^12 amplitudes on either
    side are uploaded and downloaded."""
    n, w = 12, 1 << 12
    off_s, off_d = 1234 * w, 4321 * w
    win_s, win_d = _rand_state(n + 2, 74)[:3 * w], _rand_state(n + 2, 75)[:3 * w]       # left guard | view | right guard
    psi = win_s[w:2 * w]
    lists = _families(n, 76)
    x, z, co = _arrays(lists["weights"] + lists["wide"] + lists["breaks"] + lists["z_outside"], np.random.default_rng(77))
    tiles = [int(t) for t in plan_expectation(n, x)[1]]
    assert len(tiles) >= 4 and 0 in tiles and tiles[0] != 0
    a, b = DeviceChunk.empty(25), DeviceChunk.empty(25)
    src, dst = a.view(off_s, n), b.view(off_d, n)
    try:
        a.upload(win_s, offset=off_s - w)
        b.upload(win_d, offset=off_d - w)
        dst.profile_begin()
        passes = dst.apply_pauli_sum(src, x, z, co)
        entry = [e for e in dst.profile_end() if e["kernel"].startswith("k_psum")]
        assert passes == len(tiles)
        assert len(entry) == 1 and entry[0]["launches"] == entry[0]["streaming_launches"] == passes, entry
        assert entry[0]["algorithmic_bytes"] == entry[0]["hbm_bytes"] == 32.0 * w + 48.0 * w * (passes - 1), entry
        got = b.download(off_d - w, 3 * w)
        want = apply_sum(psi, x, z, co)
        assert float(np.max(np.abs(got[w:2 * w] - want))) < ATOL
        assert got[:w].tobytes() == win_d[:w].tobytes() and got[2 * w:].tobytes() == win_d[2 * w:].tobytes()
        assert a.download(off_s - w, 3 * w).tobytes() == win_s.tobytes()
        # <H psi|P_t|psi>: dst is the bra now
        src.profile_begin()
        me = src.overlap_pauli(dst, x, z)
        entry = [e for e in src.profile_end() if e["kernel"].startswith("k_ovl")]
        assert len(entry) == 1 and entry[0]["launches"] == entry[0]["streaming_launches"] == passes == src.last_overlap_passes, entry
        assert entry[0]["algorithmic_bytes"] == entry[0]["hbm_bytes"] == 32.0 * w * passes, entry
        assert float(np.max(np.abs(me - matrix_elements(want, psi, x, z)))) < ATOL
        assert a.download(off_s - w, 3 * w).tobytes() == win_s.tobytes()
        assert b.download(off_d - w, 3 * w).tobytes() == got.tobytes()
    finally:
        src.close()
        dst.close()
        a.close()
        b.close()


def test_views():
    psi, other = _rand_state(14, 78), _rand_state(10, 79)
    lists = _families(10, 80)
    x, z, co = _arrays(lists["singles"] + lists["weights"] + lists["top"], np.random.default_rng(81))
    c, src = DeviceChunk.empty(14), DeviceChunk.from_numpy(other)
    try:
        for off in (0, 3 << 10, 15 << 10):
            c.upload(psi)
            v = c.view(off, 10)
            try:
                assert v.apply_pauli_sum(src, x, z, co) == 1
                me = src.overlap_pauli(v, x, z)                      # the view as the bra
            finally:
                v.close()
            got = c.download()
            want = apply_sum(other, x, z, co)
            assert float(np.max(np.abs(got[off:off + 1024] - want))) < ATOL, off
            assert float(np.max(np.abs(me - matrix_elements(want, other, x, z)))) < ATOL, off
            outside = np.ones(1 << 14, dtype=bool)
            outside[off:off + 1024] = False
            assert got[outside].tobytes() == psi[outside].tobytes(), off      # the parent outside the view: bitwise unchanged
        # two views of one parent, src and dst side by side
        c.upload(psi)
        s, d = c.view(5 << 10, 10), c.view(6 << 10, 10)
        try:
            assert d.apply_pauli_sum(s, x, z, co) == 1
        finally:
            s.close()
            d.close()
        got = c.download()
        assert float(np.max(np.abs(got[6 << 10:7 << 10] - apply_sum(psi[5 << 10:6 << 10], x, z, co)))) < ATOL
        outside = np.ones(1 << 14, dtype=bool)
        outside[6 << 10:7 << 10] = False
        assert got[outside].tobytes() == psi[outside].tobytes()
    finally:
        c.close()
        src.close()


# ---- refused calls ----------------------------------------------------------------------------------------------------
def test_errors():
    from tests.test_gpu_kernels import _random_ops
    k = 12
    psi, phi = _rand_state(k, 82), _rand_state(k, 83)
    lib = _lib.load()
    dst, src, buf = DeviceChunk.from_numpy(phi), DeviceChunk.from_numpy(psi), DeviceChunk.empty(k)
    small = DeviceChunk.from_numpy(_rand_state(k - 1, 84))
    whole = dst.view(0, k)                                           # the same range as dst through another handle
    elsewhere = DeviceChunk.wrap_pointer(src.device_ptr, k, device=1)              # another device (nothing is launched)
    foreign = DeviceChunk.wrap_pointer(src.device_ptr, k, device=0, stream=0)      # the null stream, not the library's
    try:
        def arrays(x, z, co):
            return [None if a is None else np.array(a, dtype=t) for a, t in ((x, np.uint64), (z, np.uint64), (co, np.float64))]

        def psum(x, z, co, n=None, passes=True, d=dst._h, s=src._h):
            xs, zs, cs = arrays(x, z, co)
            out = C.c_int(-1)
            return lib.qsim_apply_pauli_sum(d, s, 2 if n is None else n, _lib.ptr(xs), _lib.ptr(zs), _lib.ptr(cs), C.byref(out) if passes else None)

        def ovl(x, z, n=None, passes=True, out=True, kt=dst._h, br=src._h):
            xs, zs, _ = arrays(x, z, None)
            res, cnt = np.zeros(4), C.c_int(-1)
            return lib.qsim_overlap_pauli(kt, br, 2 if n is None else n, _lib.ptr(xs), _lib.ptr(zs), _lib.ptr(res) if out else None,
                                          C.byref(cnt) if passes else None)

        def unchanged():
            assert dst.download().tobytes() == phi.tobytes() and src.download().tobytes() == psi.tobytes()

        ok = ([1, 2], [0, 4], [0.25, -0.75])
        INV, NONLOCAL = _lib.QSIM_ERR_INVALID, _lib.QSIM_ERR_NONLOCAL
        for xm, zm in ((1 << k, 0), (0, 1 << (k + 1)), (1, 1 << 63)):
            assert psum([1, xm], [0, zm], ok[2]) == NONLOCAL
            assert ovl([1, xm], [0, zm]) == NONLOCAL
        for bad in (float("nan"), float("inf"), -float("inf")):
            assert psum(ok[0], ok[1], [0.1, bad]) == INV
        assert psum(None, ok[1], ok[2]) == INV and psum(ok[0], None, ok[2]) == INV and psum(ok[0], ok[1], None) == INV
        assert psum(*ok, passes=False) == INV and psum(*ok, d=None) == INV and psum(*ok, s=None) == INV
        assert psum(*ok, n=-1) == INV
        assert ovl(None, ok[1]) == INV and ovl(ok[0], None) == INV and ovl(ok[0], ok[1], out=False) == INV
        assert ovl(ok[0], ok[1], passes=False) == INV and ovl(ok[0], ok[1], kt=None) == INV and ovl(ok[0], ok[1], br=None) == INV
        assert ovl(ok[0], ok[1], n=-1) == INV
        unchanged()
        # the pair: size, device, stream
        for other in (small, elsewhere, foreign):
            assert psum(*ok, s=other._h) == INV and psum(*ok, d=other._h, s=dst._h) == INV
            assert ovl(ok[0], ok[1], br=other._h) == INV and ovl(ok[0], ok[1], kt=other._h, br=dst._h) == INV
        assert psum(*ok, s=elsewhere._h) == INV and "devices" in lib.qsim_last_error().decode()
        assert psum(*ok, s=foreign._h) == INV and "streams" in lib.qsim_last_error().decode()
        unchanged()
        # overlapping ranges: refused out of place, allowed where both chunks are only read
        assert psum(*ok, s=dst._h) == INV and psum(*ok, s=whole._h) == INV and psum(*ok, d=whole._h, s=dst._h) == INV
        assert "overlap" in lib.qsim_last_error().decode()
        assert ovl(ok[0], ok[1], br=dst._h) == _lib.QSIM_OK and ovl(ok[0], ok[1], br=whole._h) == _lib.QSIM_OK
        unchanged()
        # the wrappers
        with pytest.raises(NotImplementedError):
            dst.apply_pauli_sum(src, [1 << k], [0], [1.0])
        with pytest.raises(NotImplementedError):
            dst.overlap_pauli(src, [0], [1 << k])
        with pytest.raises(ValueError):
            dst.apply_pauli_sum(src, [1], [0], [float("nan")])
        with pytest.raises(ValueError):
            dst.apply_pauli_sum(src, [1, 2], [0], [0.5, 0.5])
        with pytest.raises(ValueError):
            dst.overlap_pauli(src, [1, 2], [0])
        with pytest.raises(ValueError):
            dst.apply_pauli_sum(dst, [1], [0], [1.0])
        with pytest.raises(ValueError):
            dst.apply_pauli_sum(small, [1], [0], [1.0])
        with pytest.raises(ValueError):
            dst.overlap_pauli(small, [1], [0])
        unchanged()
        # a split qsim_apply_ops_io has left pieces pending on a chunk: refused on either side
        src.apply_ops_io(_random_ops(k, 10, 1), dst=(buf, [5], None, -1), parts=-2)
        assert src.pending_parts()
        for call in (lambda: dst.apply_pauli_sum(src, *ok), lambda: src.overlap_pauli(dst, ok[0], ok[1]),
                     lambda: dst.overlap_pauli(src, ok[0], ok[1])):
            with pytest.raises(ValueError, match="pending"):
                call()
        assert dst.download().tobytes() == phi.tobytes()
        for j in range(len(src.pending_parts())):
            src.store_part(j)
        dst.apply_ops_io(_random_ops(k, 10, 2), dst=(buf, [5], None, -1), parts=-2)
        assert dst.pending_parts()
        with pytest.raises(ValueError, match="pending"):
            dst.apply_pauli_sum(src, *ok)
        for j in range(len(dst.pending_parts())):
            dst.store_part(j)
        assert psum(*ok) == _lib.QSIM_OK and ovl(ok[0], ok[1]) == _lib.QSIM_OK
        assert psum(None, None, None, n=0) == _lib.QSIM_OK and ovl(None, None, n=0, out=False) == _lib.QSIM_OK
    finally:
        elsewhere._h = C.c_void_p()                                  # (not destroyed: qsim_destroy would select device 1)
        for c in (whole, foreign, small, buf, src, dst):
            c.close()


# ---- the engine and the runner ----------------------------------------------------------------------------------------
def _hamiltonian(n, seed):
    """Chain bonds, the identity and one all-X string (wider than a tile at n = 12), sum |c_t| = 1."""
    rng = np.random.default_rng(seed)
    terms = [(float(rng.uniform(0.5, 1.5)), {q: p, q + 1: p}) for q in range(n - 1) for p in "XYZ"]
    terms += [(0.4, {}), (0.3, {0: "Z", n - 1: "Y"}), (-0.6, {q: "X" for q in range(n)})]
    total = sum(abs(c) for c, _ in terms)
    return PauliSum([(c / total, ops) for c, ops in terms], n_qubits=n)


def _rotations(n, count, seed):
    """`count` rotations over LOGICAL qubits: random strings, the all-X string (a wide pass) and a repeated string."""
    rng = np.random.default_rng(seed)
    full = (1 << n) - 1
    x = [int(v) for v in rng.integers(0, full + 1, count)]
    z = [int(v) for v in rng.integers(0, full + 1, count)]
    x[3], z[3] = full, 0
    x[5], z[5] = 1 << 4, 0
    x[9], z[9] = 0, 3 << (n - 2)
    x[count - 1], z[count - 1] = x[0], z[0]
    return np.array(x, dtype=np.uint64), np.array(z, dtype=np.uint64), rng.uniform(-np.pi, np.pi, count)


def _check_variance_and_gradient(psi, H, rot, variance, gradient, state_after):
    hpsi = apply_sum(psi, H.x, H.z, H.coeffs)
    mean = float(np.vdot(psi, hpsi).real)
    got = variance()
    assert abs(got - (float(np.vdot(hpsi, hpsi).real) - mean * mean)) < ATOL
    energy, grad = gradient()
    want_e, want = gradient_forward(psi, *rot, H.x, H.z, H.coeffs)
    err = float(np.max(np.abs(grad - want)))
    print(f"gradient over {len(want)} rotations: max |got - want| = {err:.3e} (bound {GRAD_ATOL:g}), |E - want| = {abs(energy - want_e):.3e}")
    assert grad.shape == want.shape and err < GRAD_ATOL
    assert abs(energy - want_e) < ATOL
    assert float(np.max(np.abs(want))) > 1e-2
    back = float(np.max(np.abs(state_after() - psi)))
    print(f"state after the backward sweep: max |after - before| = {back:.3e} (bound 1e-13)")
    assert back < 1e-13


@pytest.mark.parametrize("staged", [False, True], ids=["identity", "staged"])
def test_engine(staged):
    from quantum_simulations_amd.runner.engine import SingleGpuEngine
    n = 12
    eng = SingleGpuEngine(n, layout="search" if staged else "identity")
    other = DeviceChunk.empty(n)
    try:
        eng.init_zero_state()
        eng.execute(eng.plan(gen.random_1q_cx_circuit(n, depth=6, seed=9), repeats=8 if staged else 1))
        if staged:
            l2p = [int(p) for p in np.random.default_rng(3).permutation(n)]
            eng._adopt_layout(l2p)                                   # (SWAP passes: the state now lives in that layout)
            assert eng.l2p == l2p
        else:
            assert eng.l2p is None or eng.l2p == list(range(n))
        layout = eng.l2p
        logical = (lambda v: v) if layout is None else (lambda v: permute_state(v, layout))
        H, rot = _hamiltonian(n, 4), _rotations(n, 24, 5)
        psi = eng.state_vector()
        hpsi = apply_sum(psi, H.x, H.z, H.coeffs)
        out = eng.apply_observable(H)
        assert out is eng._work and out.last_pauli_sum_passes >= 2              # the all-X string has a wide pass
        assert float(np.max(np.abs(logical(out.download()) - hpsi))) < ATOL
        assert eng.apply_observable(H, out=other) is other
        assert float(np.max(np.abs(logical(other.download()) - hpsi))) < ATOL
        assert abs(eng.overlap_with(other, None) - np.vdot(hpsi, psi)) < ATOL    # <H psi|psi>
        assert abs(eng.overlap_with(other, H) - np.vdot(hpsi, hpsi)) < ATOL      # <H psi|H|psi>
        _check_variance_and_gradient(psi, H, rot, lambda: eng.variance(H), lambda: eng.gradient(rot, H), eng.state_vector)
        assert eng.l2p == layout and not eng._zero                  # the state did not move
    finally:
        other.close()
        eng.close()
        assert eng._work is None


@pytest.mark.parametrize("staged", [False, True], ids=["identity", "staged"])
def test_single_node(staged):
    from quantum_simulations_amd.runner import single_node
    n = 12
    buf = single_node.run(gen.random_1q_cx_circuit(n, depth=8, seed=5), chunk_size=1 << 9, use_fusion=True, use_staging=staged)
    try:
        l2p = getattr(buf, "log_to_phys", None) or None
        if staged:
            assert l2p and l2p != list(range(n))
        else:
            assert l2p is None or l2p == list(range(n))
        logical = (lambda v: v) if l2p is None else (lambda v: permute_state(v, l2p))
        psi = logical(buf.state.download())
        H, rot = _hamiltonian(n, 7), _rotations(n, 24, 8)
        _check_variance_and_gradient(psi, H, rot, lambda: single_node.variance(buf, H), lambda: single_node.gradient(buf, rot, H),
                                     lambda: logical(buf.state.download()))
        assert (getattr(buf, "log_to_phys", None) or None) == l2p
    finally:
        buf.close()
