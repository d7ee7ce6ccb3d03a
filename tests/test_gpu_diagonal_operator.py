"""qsim_apply_diagonal_sum and qsim_overlap_diagonal on an MI355X against tests/diagonal_operator_reference, over the ten
list families of tests/test_gpu_diagonal.py, then `qaoa_gradient` and the `fuse_diagonal` paths through the engine and the
runner.

Bounds.  States have unit norm, so |amplitude| <= 1.  E(i) is a sum of T terms of total weight S = sum|c_t| followed by 11
add/sub stages, each rounding relative to S: about (11 + log2 T) eps S <= 25 * 1.1e-16 * S = 3e-15 S, and dst = E src (one
product) or dst + E src (one fma) adds an eps of the result.  The bound is the project's 1e-12, relative to S as in the
moments test: 1e-12 * max(1, S) absolute for amplitudes, 1e-12 for <bra|ket> and 1e-12 * S for <bra|D|ket> (sums of 2^n
products whose moduli add up to at most 1 and S)."""
import ctypes as C

import numpy as np
import pytest

from quantum_simulations_amd import _lib, diagonal, hamiltonian
from quantum_simulations_amd import circuits as gen
from quantum_simulations_amd.circuit.staging import permute_state
from quantum_simulations_amd.kernel.device import DeviceChunk
from quantum_simulations_amd.observable import PauliSum
from tests import diagonal_operator_reference as dref
from tests import diagonal_reference as ref
from tests.krylov_reference import ising_chain
from tests.test_gpu_diagonal import _lists, _rand_state, _subset

pytestmark = pytest.mark.gpu

ATOL = 1e-12
GRAD_ATOL = 1e-11                     # tests/test_gpu_hamiltonian.py
K_APPLY = "k_diag_apply diagonal Pauli sum applied"
K_OVERLAP = "k_diag_overlap diagonal matrix element"
WEIGHTS = [0.5, 3.0, 20.0]            # sum |c_t| of the compared lists, in turn


def _coeffs(rng, name, count, weight):
    c = rng.standard_normal(count)
    if name == "zero_coefficients":
        c[::3] = 0.0
    return c * (weight / float(np.sum(np.abs(c))))


def _check(dst, src, psi, phi, z, co, what):
    """Write, accumulate, in place and the overlaps for one list; dst holds phi and src holds psi on entry and on return."""
    n = psi.size.bit_length() - 1
    s = float(np.sum(np.abs(co)))
    bound = ATOL * max(1.0, s)
    e = ref.energies(n, z, co)                                   # once per list, shared by every check below
    want = e * psi
    dst.apply_diagonal_sum(src, z, co)
    first = dst.download()
    err_w = float(np.max(np.abs(first - want)))
    assert src.download().tobytes() == psi.tobytes(), what       # src is only read
    dst.apply_diagonal_sum(src, z, co)
    assert dst.download().tobytes() == first.tobytes(), what     # the same bits twice
    dst.upload(phi)
    dst.apply_diagonal_sum(src, z, co, accumulate=True)
    err_a = float(np.max(np.abs(dst.download() - (phi + want))))
    assert src.download().tobytes() == psi.tobytes(), what
    dst.upload(psi)
    dst.apply_diagonal_sum(dst, z, co)                           # in place
    err_i = float(np.max(np.abs(dst.download() - want)))
    dst.upload(phi)
    # overlaps: src is the ket, dst the bra
    ov, el = src.overlap_diagonal(dst, z, co)
    want_ov, want_el = complex(np.vdot(phi, psi)), complex(np.vdot(phi, want))
    again = src.overlap_diagonal(dst, z, co)
    assert np.array([ov, el]).tobytes() == np.array(again).tobytes(), what
    same_ov, same_el = src.overlap_diagonal(src, z, co)
    n2, m1, _ = src.diagonal_moments(z, co)
    print(f"{what}: {z.size} terms, sum|c| = {s:.3g}: write {err_w:.2e}, accumulate {err_a:.2e}, in place {err_i:.2e} (bound {bound:.1e}); "
          f"<bra|ket> {abs(ov - want_ov):.2e} (bound {ATOL:g}), <bra|D|ket> {abs(el - want_el):.2e} (bound {ATOL * s:.1e}); "
          f"bra = ket against the moments: {abs(same_ov - n2):.2e}, {abs(same_el - m1):.2e}")
    assert err_w < bound and err_a < bound and err_i < bound, (what, err_w, err_a, err_i)
    assert abs(ov - want_ov) < ATOL and abs(el - want_el) < ATOL * s, what
    assert abs(same_ov.real - n2) < ATOL and abs(same_el.real - m1) < ATOL * s, what
    assert abs(same_ov.imag) < ATOL and abs(same_el.imag) < ATOL * s, what
    assert src.download().tobytes() == psi.tobytes() and dst.download().tobytes() == phi.tobytes(), what


@pytest.mark.parametrize("n", list(range(1, 15)))
def test_against_the_reference(n):
    psi, phi = _rand_state(n, n), _rand_state(n, 100 + n)
    rng = np.random.default_rng(900 + n)
    src, dst = DeviceChunk.from_numpy(psi), DeviceChunk.from_numpy(phi)
    try:
        for i, (name, z) in enumerate(_lists(n, 300 + n).items()):
            _check(dst, src, psi, phi, z, _coeffs(rng, name, z.size, WEIGHTS[i % 3]), f"n={n} {name}")
        # no terms: zeros when writing, untouched when accumulating, the D part of the overlap exactly 0
        dst.profile_begin()
        dst.apply_diagonal_sum(src, [], [], accumulate=True)
        assert [e for e in dst.profile_end() if e["kernel"] == K_APPLY] == []
        assert dst.download().tobytes() == phi.tobytes()
        ov, el = src.overlap_diagonal(dst, [], [])
        assert abs(ov - np.vdot(phi, psi)) < ATOL and el == 0.0
        dst.apply_diagonal_sum(src, [], [])
        assert not np.any(dst.download())
        assert src.download().tobytes() == psi.tobytes()
    finally:
        src.close()
        dst.close()


def test_term_limit():
    n, T = 12, 16384
    rng = np.random.default_rng(75)
    psi, phi = _rand_state(n, 76), _rand_state(n, 77)
    z = rng.integers(0, 1 << n, size=T + 1, dtype=np.uint64)
    z[:200] = np.uint64(1 << 11)                                          # one segment of 200 + terms: pieces and a join
    co = np.append(_coeffs(rng, "", T, 3.0), 0.25)
    src, dst = DeviceChunk.from_numpy(psi), DeviceChunk.from_numpy(phi)
    try:
        _check(dst, src, psi, phi, z[:T], co[:T], f"n={n} {T} terms")
        lib = _lib.load()
        out = np.zeros(4)
        for acc in (0, 1):
            assert lib.qsim_apply_diagonal_sum(dst._h, src._h, T + 1, _lib.ptr(z), _lib.ptr(co), acc) == _lib.QSIM_ERR_INVALID
        assert lib.qsim_overlap_diagonal(src._h, dst._h, T + 1, _lib.ptr(z), _lib.ptr(co), _lib.ptr(out)) == _lib.QSIM_ERR_INVALID
        with pytest.raises(ValueError, match="16384"):
            dst.apply_diagonal_sum(src, z, co)
        with pytest.raises(ValueError, match="16384"):
            src.overlap_diagonal(dst, z, co)
        assert dst.download().tobytes() == phi.tobytes() and src.download().tobytes() == psi.tobytes()
    finally:
        src.close()
        dst.close()


def test_grid_stride_loop_at_22_qubits():
    """2^22 amplitudes: 2048 tiles, two per workgroup under the cap of 1024 workgroups, in both kernels; W is zeroed
    between a workgroup's tiles."""
    n = 22
    rng = np.random.default_rng(78)
    psi, phi = _rand_state(n, 79), _rand_state(n, 80)
    z = [1 << 21, 1 << 20, 3 << 20, (1 << 21) | 5, (1 << 20) | (1 << 10), (1 << n) - 1, 0, 1, 0x7FF, (1 << 21) | (1 << 11)]
    z += [_subset(rng, n, int(rng.integers(1, n + 1))) for _ in range(30)]
    z = np.array(z, dtype=np.uint64)
    co = _coeffs(rng, "", z.size, 3.0)
    s = float(np.sum(np.abs(co)))
    want = ref.energies(n, z, co) * psi
    src, dst = DeviceChunk.from_numpy(psi), DeviceChunk.from_numpy(phi)
    try:
        ov, el = src.overlap_diagonal(dst, z, co)
        e_ov, e_el = abs(ov - np.vdot(phi, psi)), abs(el - np.vdot(phi, want))
        dst.apply_diagonal_sum(src, z, co, accumulate=True)
        err_a = float(np.max(np.abs(dst.download() - (phi + want))))
        dst.apply_diagonal_sum(src, z, co)
        err_w = float(np.max(np.abs(dst.download() - want)))
        src.apply_diagonal_sum(src, z, co)
        err_i = float(np.max(np.abs(src.download() - want)))
        print(f"n=22: write {err_w:.2e}, accumulate {err_a:.2e}, in place {err_i:.2e} (bound {ATOL * s:.1e}); overlaps {e_ov:.2e}, {e_el:.2e}")
        assert max(err_w, err_a, err_i) < ATOL * s and e_ov < ATOL and e_el < ATOL * s
    finally:
        src.close()
        dst.close()


def test_streaming_instantiations():
    """Two 12-qubit views at different offsets inside one 2^25 allocation (512 MiB, more than the 256 MiB Infinity Cache):
    the non-temporal forms of both kernels.  Only the views and the 2^12 amplitudes on either side are moved."""
    n, w = 12, 1 << 12
    off_s, off_d = 1234 * w, 4099 * w
    win_s, win_d = _rand_state(n + 2, 81)[:3 * w], _rand_state(n + 2, 82)[:3 * w]     # left guard | view | right guard
    psi, phi = win_s[w:2 * w], win_d[w:2 * w]
    rng = np.random.default_rng(83)
    lists = _lists(n, 84)
    z = np.concatenate([lists["weights"], lists["high"], lists["long_segments"]])
    co = _coeffs(rng, "", z.size, 3.0)
    s = float(np.sum(np.abs(co)))
    want = ref.energies(n, z, co) * psi
    parent = DeviceChunk.empty(25)
    src, dst = parent.view(off_s, n), parent.view(off_d, n)

    def one_launch(kernel, bytes_per_amp):
        entry = [e for e in dst.profile_end() if e["kernel"] == kernel]
        assert len(entry) == 1 and entry[0]["launches"] == entry[0]["streaming_launches"] == 1, entry
        assert entry[0]["algorithmic_bytes"] == entry[0]["hbm_bytes"] == bytes_per_amp * w, entry

    try:
        parent.upload(win_s, offset=off_s - w)
        parent.upload(win_d, offset=off_d - w)
        dst.profile_begin()
        dst.apply_diagonal_sum(src, z, co, accumulate=True)
        one_launch(K_APPLY, 48.0)
        got = parent.download(off_d - w, 3 * w)
        assert float(np.max(np.abs(got[w:2 * w] - (phi + want)))) < ATOL * s
        assert got[:w].tobytes() == win_d[:w].tobytes() and got[2 * w:].tobytes() == win_d[2 * w:].tobytes()
        dst.profile_begin()
        ov, el = src.overlap_diagonal(dst, z, co)
        one_launch(K_OVERLAP, 32.0)
        assert abs(ov - np.vdot(got[w:2 * w], psi)) < ATOL and abs(el - np.vdot(got[w:2 * w], want)) < ATOL * s
        dst.profile_begin()
        dst.apply_diagonal_sum(src, z, co)
        one_launch(K_APPLY, 32.0)
        got = parent.download(off_d - w, 3 * w)
        assert float(np.max(np.abs(got[w:2 * w] - want))) < ATOL * s
        assert got[:w].tobytes() == win_d[:w].tobytes() and got[2 * w:].tobytes() == win_d[2 * w:].tobytes()
        assert parent.download(off_s - w, 3 * w).tobytes() == win_s.tobytes()
    finally:
        src.close()
        dst.close()
        parent.close()


def test_errors():
    from tests.test_gpu_kernels import _random_ops
    k = 12
    psi, phi = _rand_state(k, 85), _rand_state(k, 86)
    lib = _lib.load()
    dst, src, buf = DeviceChunk.from_numpy(phi), DeviceChunk.from_numpy(psi), DeviceChunk.empty(k)
    small = DeviceChunk.from_numpy(_rand_state(k - 1, 87))
    whole = dst.view(0, k)                                           # the same range as dst through another handle
    inside = dst.view(1 << (k - 1), k - 1)                           # a view inside dst: a partial overlap
    elsewhere = DeviceChunk.wrap_pointer(src.device_ptr, k, device=1)              # another device (nothing is launched)
    foreign = DeviceChunk.wrap_pointer(src.device_ptr, k, device=0, stream=0)      # the null stream, not the library's
    INV, NONLOCAL, OK = _lib.QSIM_ERR_INVALID, _lib.QSIM_ERR_NONLOCAL, _lib.QSIM_OK
    try:
        def arrays(z, co):
            return (None if z is None else np.array(z, dtype=np.uint64)), (None if co is None else np.array(co, dtype=np.float64))

        def dsum(z, co, n=None, acc=0, d=dst._h, s=src._h):
            zs, cs = arrays(z, co)
            return lib.qsim_apply_diagonal_sum(d, s, 2 if n is None else n, _lib.ptr(zs), _lib.ptr(cs), acc)

        def dovl(z, co, n=None, out=True, d=dst._h, s=src._h):     # s is the ket, d the bra
            zs, cs = arrays(z, co)
            res = np.zeros(4)
            return lib.qsim_overlap_diagonal(s, d, 2 if n is None else n, _lib.ptr(zs), _lib.ptr(cs), _lib.ptr(res) if out else None)

        def unchanged():
            assert dst.download().tobytes() == phi.tobytes() and src.download().tobytes() == psi.tobytes()

        ok = ([1, 6], [0.1, 0.2])
        for call in (dsum, dovl):
            for zm in (1 << k, 1 << (k + 1), 1 << 63):
                assert call([1, zm], ok[1]) == NONLOCAL
            assert b"index bit" in lib.qsim_last_error() and b"log2(chunk_size)=12" in lib.qsim_last_error()
            for bad in (float("nan"), float("inf"), -float("inf")):
                assert call(ok[0], [0.1, bad]) == INV
            assert call(None, ok[1]) == INV and call(ok[0], None) == INV
            assert call(*ok, d=None) == INV and call(*ok, s=None) == INV
            assert call(*ok, n=-1) == INV
            # the pair: size, device, stream
            for other in (small, elsewhere, foreign):
                assert call(*ok, s=other._h) == INV and call(*ok, d=other._h, s=dst._h) == INV
            assert call(*ok, s=elsewhere._h) == INV and "devices" in lib.qsim_last_error().decode()
            assert call(*ok, s=foreign._h) == INV and "streams" in lib.qsim_last_error().decode()
            unchanged()
        assert dovl(*ok, out=False) == INV
        for acc in (2, -1, 3):
            assert dsum(*ok, acc=acc) == INV
        assert "accumulate" in lib.qsim_last_error().decode()
        # overlapping ranges: the same range only when writing; a view inside the other never
        assert dsum(*ok, acc=1, s=dst._h) == INV and dsum(*ok, acc=1, s=whole._h) == INV and dsum(*ok, acc=1, d=whole._h, s=dst._h) == INV
        assert "overlap" in lib.qsim_last_error().decode()
        for acc in (0, 1):
            assert dsum(*ok, acc=acc, s=inside._h) == INV and dsum(*ok, acc=acc, d=inside._h, s=dst._h) == INV
        unchanged()
        assert dovl(*ok, s=dst._h) == OK and dovl(*ok, s=whole._h) == OK          # both chunks are only read
        # the wrappers
        with pytest.raises(NotImplementedError):
            dst.apply_diagonal_sum(src, [1 << k], [0.1])
        with pytest.raises(NotImplementedError):
            src.overlap_diagonal(dst, [1 << k], [0.1])
        with pytest.raises(ValueError):
            dst.apply_diagonal_sum(src, [1], [float("nan")])
        with pytest.raises(ValueError):
            src.overlap_diagonal(dst, [1], [float("nan")])
        with pytest.raises(ValueError):
            dst.apply_diagonal_sum(src, [1, 2], [0.1])
        with pytest.raises(ValueError):
            src.overlap_diagonal(dst, [1, 2], [0.1])
        with pytest.raises(ValueError):
            dst.apply_diagonal_sum(dst, *ok, accumulate=True)
        with pytest.raises(ValueError):
            dst.apply_diagonal_sum(small, *ok)
        with pytest.raises(ValueError):
            src.overlap_diagonal(small, *ok)
        unchanged()
        # a split qsim_apply_ops_io has left pieces pending on a chunk: refused on either side
        src.apply_ops_io(_random_ops(k, 10, 1), dst=(buf, [5], None, -1), parts=-2)
        assert src.pending_parts()
        for call in (lambda: dst.apply_diagonal_sum(src, *ok), lambda: dst.apply_diagonal_sum(src, *ok, accumulate=True),
                     lambda: src.overlap_diagonal(dst, *ok), lambda: dst.overlap_diagonal(src, *ok)):
            with pytest.raises(ValueError, match="pending"):
                call()
        assert dst.download().tobytes() == phi.tobytes()
        for j in range(len(src.pending_parts())):
            src.store_part(j)
        dst.apply_ops_io(_random_ops(k, 10, 2), dst=(buf, [5], None, -1), parts=-2)
        assert dst.pending_parts()
        for call in (lambda: dst.apply_diagonal_sum(src, *ok), lambda: src.overlap_diagonal(dst, *ok)):
            with pytest.raises(ValueError, match="pending"):
                call()
        for j in range(len(dst.pending_parts())):
            dst.store_part(j)
        assert dovl(*ok) == OK and dsum(*ok, acc=1) == OK and dsum(*ok) == OK and dsum(*ok, s=dst._h) == OK
        assert dsum(None, None, n=0) == OK and dsum(None, None, n=0, acc=1) == OK and dovl(None, None, n=0) == OK
    finally:
        elsewhere._h = C.c_void_p()                                  # (not destroyed: qsim_destroy would select device 1)
        for c in (inside, whole, foreign, small, buf, src, dst):
            c.close()


# ---- the engine and the runner -------------------------------------------------------------------------------------------
GAMMAS, BETAS = [2.9, -3.4], [0.7, -0.45]


def _all_pairs(n, seed):
    """Every ZZ pair with a random weight, sum |c| = 1."""
    rng = np.random.default_rng(seed)
    c = rng.standard_normal(n * (n - 1) // 2)
    c /= float(np.sum(np.abs(c)))
    pairs = [(a, b) for a in range(n) for b in range(a + 1, n)]
    return PauliSum([(float(ct), {a: "Z", b: "Z"}) for ct, (a, b) in zip(c, pairs)], n_qubits=n)


_GRADIENT = {}


def _gradient_reference(psi, cost):
    """The reference gradient of the one state and cost both gradient tests use, computed once."""
    key = psi.tobytes()
    if key not in _GRADIENT:
        _GRADIENT[key] = dref.qaoa_gradient(psi, *diagonal.diagonal_part(cost), GAMMAS, BETAS)
    return _GRADIENT[key]


def _check_gradient(got, want, what):
    energy, dg, db = got
    err = max(float(np.max(np.abs(dg - want[1]))), float(np.max(np.abs(db - want[2]))))
    print(f"{what}: |E - want| = {abs(energy - want[0]):.3e} (bound {ATOL:g}), gradient max |got - want| = {err:.3e} (bound {GRAD_ATOL:g}); "
          f"dgammas {dg}, dbetas {db}")
    assert abs(energy - want[0]) < ATOL and err < GRAD_ATOL
    assert float(np.max(np.abs(want[1]))) > 1e-3 and float(np.max(np.abs(want[2]))) > 1e-3


def test_engine_qaoa_gradient():
    from quantum_simulations_amd.runner.engine import SingleGpuEngine
    n = 12
    cost = _all_pairs(n, 11)
    eng = SingleGpuEngine(n, layout="search")
    try:
        eng.init_zero_state()
        eng.execute(eng.plan(gen.random_1q_cx_circuit(n, depth=6, seed=9), repeats=8))
        l2p = [int(p) for p in np.random.default_rng(3).permutation(n)]
        eng._adopt_layout(l2p)
        assert eng.l2p == l2p and l2p != list(range(n))
        psi = eng.state_vector()
        got = eng.qaoa_gradient(cost, GAMMAS, BETAS)
        assert eng.l2p == l2p                                                 # nothing moved
        _check_gradient(got, _gradient_reference(psi, cost), "engine qaoa_gradient n=12 p=2")
        back = float(np.max(np.abs(eng.state_vector() - psi)))
        print(f"the state after the sweep: max |after - before| = {back:.3e} (bound 1e-13)")
        assert back < 1e-13
        with pytest.raises(ValueError):
            eng.qaoa_gradient(cost, GAMMAS, BETAS[:1])
        with pytest.raises(ValueError):
            eng.qaoa_gradient(cost, [float("nan")], [0.1])
    finally:
        eng.close()


def test_single_node_qaoa_gradient():
    from quantum_simulations_amd.runner import single_node
    n = 12
    cost = _all_pairs(n, 11)
    buf = single_node.run(gen.random_1q_cx_circuit(n, depth=8, seed=5), chunk_size=1 << 9, use_fusion=True, use_staging=True)
    try:
        l2p = getattr(buf, "log_to_phys", None) or None
        assert l2p and l2p != list(range(n))
        psi = permute_state(buf.state.download(), l2p)
        got = single_node.qaoa_gradient(buf, cost, GAMMAS, BETAS)
        _check_gradient(got, _gradient_reference(psi, cost), "single_node qaoa_gradient n=12 p=2")
        assert float(np.max(np.abs(permute_state(buf.state.download(), l2p) - psi))) < 1e-13
    finally:
        buf.close()


def test_engine_fuse_diagonal(monkeypatch):
    """The transverse-field Ising chain at 12 qubits: 11 ZZ bonds go through one accumulating diagonal pass."""
    from quantum_simulations_amd.runner.engine import SingleGpuEngine
    n = 12
    H = ising_chain(n)
    monkeypatch.setattr(hamiltonian, "DIAGONAL_MIN_TERMS", n - 1)
    eng = SingleGpuEngine(n, layout="search")
    try:
        eng.init_zero_state()
        eng.execute(eng.plan(gen.random_1q_cx_circuit(n, depth=6, seed=9), repeats=8))
        eng._adopt_layout([int(p) for p in np.random.default_rng(4).permutation(n)])
        plain = eng.apply_observable(H).download()
        eng.state.profile_begin()
        fused = eng.apply_observable(H, fuse_diagonal=True).download()
        entry = [e for e in eng.state.profile_end() if e["kernel"] == K_APPLY]
        assert len(entry) == 1 and entry[0]["launches"] == 1 and entry[0]["algorithmic_bytes"] == 48.0 * (1 << n), entry
        err = float(np.max(np.abs(fused - plain)))
        v0, v1 = eng.variance(H), eng.variance(H, fuse_diagonal=True)
        print(f"apply_observable with and without fuse_diagonal: max |difference| = {err:.3e}; variance {v0:.12f} / {v1:.12f} (bound {ATOL:g})")
        assert err < ATOL and abs(v0 - v1) < ATOL
        # the Z-only part alone: the diagonal pass writes
        D = PauliSum([(-1.0, {q: "Z", q + 1: "Z"}) for q in range(n - 1)], n_qubits=n)
        plain = eng.apply_observable(D).download()
        eng.state.profile_begin()
        fused = eng.apply_observable(D, fuse_diagonal=True).download()
        entry = [e for e in eng.state.profile_end() if e["kernel"] == K_APPLY]
        assert len(entry) == 1 and entry[0]["algorithmic_bytes"] == 32.0 * (1 << n), entry
        assert float(np.max(np.abs(fused - plain))) < ATOL
    finally:
        eng.close()
    tol = 1e-8
    results = []
    for fuse in (False, True):
        eng = SingleGpuEngine(n, layout="identity")
        try:
            eng.init_random_state(5)
            eng.state.profile_begin()
            results.append(eng.ground_state(H, m=16, tol=tol, fuse_diagonal=fuse))
            assert bool([e for e in eng.state.profile_end() if e["kernel"] == K_APPLY]) == fuse
        finally:
            eng.close()
    print(f"ground_state without / with fuse_diagonal: {results[0]} / {results[1]}")
    assert results[0][1] <= tol and results[1][1] <= tol and abs(results[0][0] - results[1][0]) <= tol


def test_single_node_fuse_diagonal(monkeypatch):
    from quantum_simulations_amd.runner import single_node
    n = 12
    H = ising_chain(n)
    monkeypatch.setattr(hamiltonian, "DIAGONAL_MIN_TERMS", n - 1)
    buf = single_node.run(gen.random_1q_cx_circuit(n, depth=8, seed=5), chunk_size=1 << 9, use_fusion=True, use_staging=True)
    try:
        v0 = single_node.variance(buf, H)
        buf.state.profile_begin()
        v1 = single_node.variance(buf, H, fuse_diagonal=True)
        assert [e for e in buf.state.profile_end() if e["kernel"] == K_APPLY]
        assert abs(v0 - v1) < ATOL
        # Krylov evolution: both runs build the same 8 Lanczos vectors from H applications that differ by the rounding of
        # E, at most 3e-15 * sum|c| = 1e-13 per unit amplitude with sum|c| = 29; the recurrence divides by betas of order
        # one, so after 8 steps and the combination the states differ by a few times 8 * 1e-13: bound 1e-11
        before = buf.state.download()
        e0 = single_node.evolve_krylov(buf, H, 0.2, m=8)
        plain = buf.state.download()
        buf.state.upload(before)
        buf.state.profile_begin()
        e1 = single_node.evolve_krylov(buf, H, 0.2, m=8, fuse_diagonal=True)
        assert [e for e in buf.state.profile_end() if e["kernel"] == K_APPLY]
        diff = float(np.max(np.abs(buf.state.download() - plain)))
        print(f"evolve_krylov with and without fuse_diagonal: max |difference| = {diff:.3e} (bound 1e-11), estimates {e0:.3e} / {e1:.3e}")
        assert diff < 1e-11
        r = single_node.ground_state(buf, H, m=16, tol=1e-8, fuse_diagonal=True)
        assert r[1] <= 1e-8
    finally:
        buf.close()
