"""qsim_lincomb (dst := a_d dst + sum_s a_s src_s with <bra_b|dst> and |dst|^2 of the new dst in the same pass) on an
MI355X against the numpy reference of tests/krylov_reference.py.  States are normalised to 1 and the coefficients of a
call to sum |a| <= 1, so the project's absolute bound of 1e-12 (tests/test_gpu_hamiltonian.py) means what it means
there: an amplitude of the result is a sum of at most 5 products of total size <= 1, a dot or the norm a sum of 2^k
products of total size <= 1, each rounded to a few 1e-16."""
import ctypes as C
import itertools

import numpy as np
import pytest

from quantum_simulations_amd import _lib
from quantum_simulations_amd.kernel.device import DeviceChunk
from tests.krylov_reference import lincomb, rand_state

pytestmark = pytest.mark.gpu

ATOL = 1e-12
INV = _lib.QSIM_ERR_INVALID


def _coeffs(rng, count):
    """`count` complex coefficients with sum |a| = 1."""
    a = rng.standard_normal(count) + 1j * rng.standard_normal(count)
    return a / np.sum(np.abs(a))


def _check(got, want, what):
    dst, dots, norm2 = got
    err = float(np.max(np.abs(dst - want[0]))) if len(dst) else 0.0
    assert err < ATOL, (what, "amplitudes", err)
    assert dots.shape == want[1].shape
    if len(dots):
        assert float(np.max(np.abs(dots - want[1]))) < ATOL, (what, "dots")
    assert (norm2 is None) == (want[2] is None), what
    if norm2 is not None:
        assert abs(norm2 - want[2]) < ATOL, (what, "norm2")


@pytest.mark.parametrize("k", list(range(0, 15)))
def test_every_form_against_the_reference(k):
    """(n_src, n_bras) in 0..4 x 0..4, dst_coeff in {0, 1, general}, with and without the norm: every instantiation of
    k_lincomb's cached form.  Chunks of fewer than 1024 amplitudes (k < 10) have threads and items that load nothing.
    Every call is made twice on the same inputs: the same bits."""
    rng = np.random.default_rng(900 + k)
    d0 = rand_state(k, 10 * k)
    src_np = [rand_state(k, 10 * k + 1 + s) for s in range(4)]
    bra_np = [rand_state(k, 10 * k + 5 + b) for b in range(4)]
    nan = np.full(1 << k, np.nan + 1j * np.nan)
    dst = DeviceChunk.empty(k)
    srcs, bras = [DeviceChunk.from_numpy(v) for v in src_np], [DeviceChunk.from_numpy(v) for v in bra_np]
    try:
        worst = 0.0
        for n_src, n_bras, kind, want_norm in itertools.product(range(5), range(5), ("zero", "one", "general"), (False, True)):
            a = _coeffs(rng, n_src + 1)
            dc = {"zero": 0.0, "one": 1.0, "general": a[0]}[kind]
            # a_d = 1 exactly: dst of norm 1/2 and sum |a_s| <= 1/2 instead, so the result is of size <= 1 all the same
            co, d_in = (0.5 * a[1:], 0.5 * d0) if kind == "one" else (a[1:], d0)
            what = (k, n_src, n_bras, kind, want_norm)
            results = []
            for _ in range(2):
                dst.upload(nan if kind == "zero" else d_in)            # a_d = 0: what dst held does not matter, NaNs included
                dots, norm2 = dst.lincomb(dc, srcs[:n_src], co, bras[:n_bras], want_norm)
                results.append((dst.download(), dots, norm2))
            got, again = results
            assert got[0].tobytes() == again[0].tobytes() and got[1].tobytes() == again[1].tobytes() and got[2] == again[2], what
            assert np.all(np.isfinite(got[0])) and np.all(np.isfinite(got[1])), what
            want = lincomb(d_in, dc, src_np[:n_src], co, bra_np[:n_bras], want_norm)
            _check(got, want, what)
            worst = max(worst, float(np.max(np.abs(got[0] - want[0]))))
            if kind == "one" and n_src == 0:
                assert got[0].tobytes() == d_in.tobytes(), what        # the read-only form: dst is not written
            if kind == "zero" and n_src == 0:
                assert not np.any(got[0]), what
        for c, v in zip(srcs + bras, src_np + bra_np):                  # only read, by every call
            assert c.download().tobytes() == v.tobytes()
        print(f"k={k}: 150 forms twice, max |got - want| over the amplitudes = {worst:.3e} (bound {ATOL:g})")
    finally:
        for c in [dst] + srcs + bras:
            c.close()


def test_sources_and_bras_unchanged_after_every_call():
    k = 11
    d0, s_np, b_np = rand_state(k, 1), [rand_state(k, 2), rand_state(k, 3)], [rand_state(k, 4), rand_state(k, 5)]
    dst, srcs, bras = DeviceChunk.from_numpy(d0), [DeviceChunk.from_numpy(v) for v in s_np], [DeviceChunk.from_numpy(v) for v in b_np]
    try:
        for dc, ns, nb, norm in ((0.0, 2, 2, True), (1.0, 0, 2, True), (0.25 - 0.5j, 2, 1, False), (1.0, 1, 0, False), (0.5, 0, 0, False)):
            dst.lincomb(dc, srcs[:ns], [0.25, -0.25j][:ns], bras[:nb], norm)
            for c, v in zip(srcs + bras, s_np + b_np):
                assert c.download().tobytes() == v.tobytes(), (dc, ns, nb, norm)
        assert dst.dot(bras[0]) == dst.lincomb(1.0, bras=[bras[0]])[0][0]
        assert abs(dst.dot(bras[0]) - np.vdot(b_np[0], dst.download())) < ATOL
    finally:
        for c in [dst] + srcs + bras:
            c.close()


@pytest.mark.parametrize("k", [7, 14])
def test_a_bra_on_a_source_gives_the_same_bits_as_a_copy(k):
    d0, s0, s1, b0 = (rand_state(k, 20 + j) for j in range(4))
    dst, other = DeviceChunk.empty(k), DeviceChunk.empty(k)
    src = [DeviceChunk.from_numpy(s0), DeviceChunk.from_numpy(s1)]
    copy = [DeviceChunk.from_numpy(s0), DeviceChunk.from_numpy(s1)]
    bra = DeviceChunk.from_numpy(b0)
    try:
        co = [0.25 + 0.25j, -0.3]
        for dc in (0.0, 1.0, 0.2 - 0.1j):
            dst.upload(d0)
            other.upload(d0)
            dots_a, n_a = dst.lincomb(dc, src, co, [src[1], bra, src[0], bra], True)        # aliases, and the same bra twice
            dots_c, n_c = other.lincomb(dc, src, co, [copy[1], bra, copy[0], bra], True)
            assert dots_a.tobytes() == dots_c.tobytes() and n_a == n_c, dc
            assert dots_a[1] == dots_a[3]
            assert dst.download().tobytes() == other.download().tobytes(), dc
            _check((dst.download(), dots_a, n_a), lincomb(d0, dc, [s0, s1], co, [s1, b0, s0, b0], True), dc)
    finally:
        for c in [dst, other, bra] + src + copy:
            c.close()


def test_the_loop_path_at_23_qubits():
    """A block is kBlock * kLcItems = 256 * 4 = 1024 amplitudes and the grid is capped at kLcMaxWg = 2048 workgroups, so
    a workgroup walks 2^k / (1024 * 2048) blocks: one up to k = 21, two at k = 22, FOUR at k = 23 -- the smallest size at
    which the loop runs at least three times (first, middle and last block of a workgroup).  Three chunks of 128 MiB
    filled on the device; two sources with the bras aliasing them."""
    k = 23
    dst, s0, s1 = DeviceChunk.empty(k), DeviceChunk.empty(k), DeviceChunk.empty(k)
    try:
        for j, c in enumerate((dst, s0, s1)):
            c.init_random(40 + j)
        d_np, s_np = dst.download(), [s0.download(), s1.download()]
        dc, co = 0.3 - 0.2j, [0.25j, -0.35]
        want = lincomb(d_np, dc, s_np, co, s_np, True)
        dots, norm2 = dst.lincomb(dc, [s0, s1], co, [s0, s1], True)
        got = dst.download()
        err = float(np.max(np.abs(got - want[0])))
        print(f"k=23: max |got - want| = {err:.3e}, dots {np.max(np.abs(dots - want[1])):.3e}, norm2 {abs(norm2 - want[2]):.3e} (bound {ATOL:g})")
        _check((got, dots, norm2), want, "k=23")
        again = dst.lincomb(1.0, bras=[s0, s1], want_norm2=True)                  # the read-only form over the new dst
        assert float(np.max(np.abs(again[0] - want[1]))) < ATOL and abs(again[1] - want[2]) < ATOL
        assert dst.download().tobytes() == got.tobytes()
    finally:
        for c in (dst, s0, s1):
            c.close()


def test_streaming_instantiations():
    """12-qubit views inside two 2^25-amplitude allocations (512 MiB each, more than the 256 MiB Infinity Cache): the
    non-temporal forms.  Only the views and the 2^12 amplitudes on either side of dst are uploaded and downloaded.  The
    result is bitwise what the same call gives on small, cached chunks; hbm_bytes = 16 B per amplitude for every stream
    read (a bra on a source counted once) + 16 B if dst is written."""
    k, w = 12, 1 << 12
    off_d, offs = 4321 * w, [1234 * w, 77 * w, 5000 * w, 8000 * w]
    win_d = rand_state(k + 2, 50)[:3 * w]                                         # left guard | view | right guard
    d0 = win_d[w:2 * w]
    vec = [rand_state(k, 51 + j) for j in range(4)]
    a, b = DeviceChunk.empty(25), DeviceChunk.empty(25)
    dst = b.view(off_d, k)
    far = [a.view(o, k) for o in offs[:3]] + [b.view(offs[3], k)]                 # three views of the other allocation, one of dst's
    small_dst, small = DeviceChunk.empty(k), [DeviceChunk.from_numpy(v) for v in vec]
    try:
        for v, c in zip(vec, far):
            c.upload(v)
        # (dst_coeff, sources, bras, norm) -> streams read, dst written
        forms = [((0.25 - 0.25j), [0, 1], [1, 2, 3], True, 5, 1),                 # dst, 2 sources, 2 bras of their own
                 (0.0, [2], [2], False, 1, 1),                                     # dst not read, the bra is the source
                 (1.0, [], [0, 3], True, 3, 0),                                    # read-only
                 (1.0, [0, 1, 2, 3], [], False, 5, 1),                             # no reduction: only enqueued
                 (0.0, [], [], False, 0, 1)]                                       # fill with zeros
        for dc, si, bi, norm, reads, writes in forms:
            co = _coeffs(np.random.default_rng(len(si)), max(len(si), 1))[:len(si)] * 0.5
            b.upload(win_d, offset=off_d - w)
            small_dst.upload(d0)
            dst.profile_begin()
            dots, n2 = dst.lincomb(dc, [far[j] for j in si], co, [far[j] for j in bi], norm)
            entry = [e for e in dst.profile_end() if e["kernel"].startswith("k_lincomb")]
            assert len(entry) == 1 and entry[0]["kernel"] == "k_lincomb linear combination", entry
            assert entry[0]["launches"] == entry[0]["streaming_launches"] == 1, entry
            assert entry[0]["algorithmic_bytes"] == entry[0]["hbm_bytes"] == 16.0 * w * (reads + writes), entry
            small_dst.profile_begin()
            dots_s, n2_s = small_dst.lincomb(dc, [small[j] for j in si], co, [small[j] for j in bi], norm)
            entry = [e for e in small_dst.profile_end() if e["kernel"].startswith("k_lincomb")]
            assert len(entry) == 1 and entry[0]["launches"] == 1 and entry[0]["streaming_launches"] == 0, entry
            got = b.download(off_d - w, 3 * w)
            assert got[:w].tobytes() == win_d[:w].tobytes() and got[2 * w:].tobytes() == win_d[2 * w:].tobytes()
            assert got[w:2 * w].tobytes() == small_dst.download().tobytes()
            assert dots.tobytes() == dots_s.tobytes() and n2 == n2_s
            want = lincomb(d0, dc, [vec[j] for j in si], co, [vec[j] for j in bi], norm)
            assert float(np.max(np.abs(got[w:2 * w] - want[0]))) < ATOL
            for v, c in zip(vec, far):
                assert c.download().tobytes() == v.tobytes()
        # nothing to write and nothing to reduce: no launch at all
        dst.profile_begin()
        dst.lincomb(1.0)
        assert not [e for e in dst.profile_end() if e["kernel"].startswith("k_lincomb")]
    finally:
        for c in [dst, small_dst] + far + small + [a, b]:
            c.close()


def test_views():
    """Views at the first, a middle and the last offset of a parent as dst, and dst and a source as neighbouring views of
    one parent: the parent outside dst is bitwise unchanged."""
    K, k, w = 14, 10, 1 << 10
    psi, other, third = rand_state(K, 60), rand_state(k, 61), rand_state(k, 62)
    c, src, bra = DeviceChunk.empty(K), DeviceChunk.from_numpy(other), DeviceChunk.from_numpy(third)
    try:
        dc, co = 0.4j, [0.3 - 0.3j]
        for off in (0, 3 * w, 15 * w):
            c.upload(psi)
            v = c.view(off, k)
            try:
                dots, n2 = v.lincomb(dc, [src], co, [bra, src], True)
            finally:
                v.close()
            got = c.download()
            _check((got[off:off + w], dots, n2), lincomb(psi[off:off + w], dc, [other], co, [third, other], True), off)
            outside = np.ones(1 << K, dtype=bool)
            outside[off:off + w] = False
            assert got[outside].tobytes() == psi[outside].tobytes(), off
        c.upload(psi)
        s, d, same = c.view(5 * w, k), c.view(6 * w, k), c.view(6 * w, k)
        try:
            dots, n2 = d.lincomb(dc, [s, src], [0.2, -0.1j], [s], True)
            with pytest.raises(ValueError, match="overlap"):
                d.lincomb(dc, [same], [1.0])                                       # dst's range through another handle
        finally:
            s.close()
            d.close()
            same.close()
        got = c.download()
        _check((got[6 * w:7 * w], dots, n2), lincomb(psi[6 * w:7 * w], dc, [psi[5 * w:6 * w], other], [0.2, -0.1j], [psi[5 * w:6 * w]], True), "side by side")
        outside = np.ones(1 << K, dtype=bool)
        outside[6 * w:7 * w] = False
        assert got[outside].tobytes() == psi[outside].tobytes()
    finally:
        for x in (c, src, bra):
            x.close()


def test_refused_calls():
    from tests.test_gpu_kernels import _random_ops
    k = 12
    d0, s0, b0 = rand_state(k, 70), rand_state(k, 71), rand_state(k, 72)
    lib = _lib.load()
    dst, src, bra, buf = DeviceChunk.from_numpy(d0), DeviceChunk.from_numpy(s0), DeviceChunk.from_numpy(b0), DeviceChunk.empty(k)
    small = DeviceChunk.from_numpy(rand_state(k - 1, 73))
    whole, inside = dst.view(0, k), dst.view(1 << (k - 1), k - 1)                 # dst's range through another handle; a view inside
    half = src.view(0, k - 1)
    elsewhere = DeviceChunk.wrap_pointer(src.device_ptr, k, device=1)              # another device (nothing is launched)
    foreign = DeviceChunk.wrap_pointer(src.device_ptr, k, device=0, stream=0)      # the null stream, not the library's
    try:
        def handles(cs):
            return (C.c_void_p * max(len(cs), 1))(*[None if c is None else c._h.value for c in cs])

        def call(d=dst, dc=(0.5, -0.25), srcs=(src,), co=(0.25, 0.5), bras=(bra,), n_src=None, n_bras=None, src_list=True,
                 co_list=True, bra_list=True, dots=True, norm=True):
            dcp = None if dc is None else np.array(dc, dtype=np.float64)
            cop = np.array(co, dtype=np.float64)
            out, n2 = np.zeros(8), C.c_double(-1.0)
            return lib.qsim_lincomb(None if d is None else d._h, _lib.ptr(dcp), len(srcs) if n_src is None else n_src,
                                    handles(srcs) if src_list else None, _lib.ptr(cop) if co_list else None,
                                    len(bras) if n_bras is None else n_bras, handles(bras) if bra_list else None,
                                    _lib.ptr(out) if dots else None, C.byref(n2) if norm else None)

        def unchanged():
            assert dst.download().tobytes() == d0.tobytes() and src.download().tobytes() == s0.tobytes()
            assert bra.download().tobytes() == b0.tobytes()

        # null required arguments (a null norm2 is fine: see the end)
        assert call(d=None) == INV and call(dc=None) == INV and call(src_list=False) == INV and call(co_list=False) == INV
        assert call(bra_list=False) == INV and call(dots=False) == INV
        assert call(srcs=(None,)) == INV and call(bras=(bra, None)) == INV
        # counts out of range
        five = (src,) * 5
        assert call(srcs=five, co=(0.1,) * 10) == INV and call(bras=five) == INV and call(n_src=-1) == INV and call(n_bras=-1) == INV
        # coefficients that are not finite
        for bad in (float("nan"), float("inf"), -float("inf")):
            assert call(dc=(bad, 0.0)) == INV and call(dc=(0.0, bad)) == INV and call(co=(bad, 0.0)) == INV and call(co=(0.0, bad)) == INV
        unchanged()
        # size, device, stream: on either side, as a source and as a bra
        for other in (small, elsewhere, foreign):
            assert call(srcs=(other,)) == INV and call(bras=(other,)) == INV and call(bras=(bra, other)) == INV
            assert call(d=other) == INV
        assert call(srcs=(elsewhere,)) == INV and "devices" in lib.qsim_last_error().decode()
        assert call(bras=(foreign,)) == INV and "streams" in lib.qsim_last_error().decode()
        unchanged()
        # a source or a bra that overlaps dst at all
        for other in (dst, whole):
            assert call(srcs=(other,)) == INV and call(bras=(other,)) == INV
            assert "overlap" in lib.qsim_last_error().decode()
        assert call(d=inside, srcs=(half,), bras=(whole.view(0, k - 1),)) == _lib.QSIM_OK     # both halves of dst: disjoint
        dst.upload(d0)
        assert call(d=inside, srcs=(half,), bras=(whole.view(1 << (k - 1), k - 1),)) == INV and "overlap" in lib.qsim_last_error().decode()
        assert call(d=whole, srcs=(src,), bras=(dst,)) == INV
        unchanged()
        # the wrapper
        with pytest.raises(ValueError):
            dst.lincomb(1.0, [src], [0.5, 0.5])
        with pytest.raises(ValueError):
            dst.lincomb(1.0, [src] * 5, [0.1] * 5)
        with pytest.raises(ValueError):
            dst.lincomb(float("nan"))
        with pytest.raises(ValueError):
            dst.lincomb(1.0, bras=[dst])
        with pytest.raises(ValueError):
            dst.dot(small)
        unchanged()
        # a split qsim_apply_ops_io has left pieces pending on a chunk: refused wherever that chunk stands
        src.apply_ops_io(_random_ops(k, 10, 1), dst=(buf, [5], None, -1), parts=-2)
        assert src.pending_parts()
        for made in (lambda: dst.lincomb(1.0, [src], [0.5]), lambda: dst.lincomb(1.0, bras=[src]), lambda: src.lincomb(0.5),
                     lambda: src.lincomb(1.0, [dst], [0.5], [bra], True)):
            with pytest.raises(ValueError, match="pending"):
                made()
        assert dst.download().tobytes() == d0.tobytes() and bra.download().tobytes() == b0.tobytes()
        for j in range(len(src.pending_parts())):
            src.store_part(j)
        # what is fine: a null norm2 with bras, no sources and no bras with null lists, sources that overlap each other
        assert call(norm=False) == _lib.QSIM_OK
        assert call(srcs=(), bras=(), src_list=False, co_list=False, bra_list=False, dots=False) == _lib.QSIM_OK
        assert call(srcs=(src, src), co=(0.1, 0.0, 0.0, 0.1), bras=(src, bra, bra)) == _lib.QSIM_OK
    finally:
        elsewhere._h = C.c_void_p()                                  # (not destroyed: qsim_destroy would select device 1)
        for c in (whole, inside, half, foreign, small, buf, src, bra, dst):
            c.close()
