"""qsim_apply_pauli_rotations on an MI355X against the host reference tests/rotation_reference.rotate (R = exp(-i theta P)
= cos(theta) I - i sin(theta) P, no factor 1/2) at 1e-12 absolute on unit-norm states, the project's bound for gate
parity at n <= 14; at most 128 rotations per compared call (1531 in the one test of the pass split at 1024), so rounding
(a few 1e-16 per rotation) stays orders below the bound.  Every single-qubit Pauli, random strings of every weight, Z outside the tile, X on the top bits, pass
breaks, strings wider than a tile; the order of non-commuting rotations; inverse, norm and bitwise repeatability; the
gate path; views; the grid-stride loop (n = 22); the streaming instantiation; errors; the engine and the runner."""
import ctypes as C

import numpy as np
import pytest

from quantum_simulations_amd import _lib, evolution
from quantum_simulations_amd import circuits as gen
from quantum_simulations_amd.circuit.staging import permute_state
from quantum_simulations_amd.kernel.device import DeviceChunk
from quantum_simulations_amd.kernel.planner import plan_pauli_rotations
from quantum_simulations_amd.observable import PauliSum
from tests.rotation_reference import LONG_N, LONG_TILE, long_rotation_list, rotate_list, rotation_gates

pytestmark = pytest.mark.gpu

ATOL = 1e-12


def _rand_state(n, seed):
    rng = np.random.default_rng(seed)
    psi = rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)
    return psi / np.linalg.norm(psi)


def _string(rng, qubits):
    x = z = 0
    for q in qubits:
        bx, bz = ((1, 0), (1, 1), (0, 1))[int(rng.integers(3))]
        x |= bx << int(q)
        z |= bz << int(q)
    return x, z


def _lists(n, seed):
    """{name: [(x, z)]}: the rotation lists of the issue for a chunk of n qubits, each of at most 128 entries."""
    rng = np.random.default_rng(seed)
    full = (1 << n) - 1
    out = {"singles": [(0, 0)] + [(bx << q, bz << q) for q in range(n) for bx, bz in ((1, 0), (1, 1), (0, 1))]}
    out["weights"] = [_string(rng, rng.choice(n, size=w, replace=False)) for w in range(1, n + 1) for _ in range(3)]
    out["identity"] = [(0, 0), (0, 0)]
    # X / Y on the top bits with a low one: from n = 12 on the tile bits are not contiguous
    t1, t2 = 1 << (n - 1), 1 << max(n - 2, 0)
    out["top"] = [(t1 | 1, int(rng.integers(0, full + 1))), (t1 | (1 << (n // 2)), t1), (t1 | t2, int(rng.integers(0, full + 1))),
                  ((t1 | t2 | 2) & full, (t1 | 2) & full)]
    if n >= 12:
        hi = full & ~0x7FF                                 # the bits a tile of the low 11 leaves outside
        out["z_outside"] = [(0, hi), (0, 1 << (n - 1)), (1 << 4, hi), (0x7F8, hi | 0x10), (3 << 5, (1 << 11) | (1 << 6)), (0, full)]
        # pass breaks: the unions of consecutive x exceed 11 bits with the line bits; x = 0 never breaks
        out["breaks"] = [(0x7F8, 0), (1 << (n - 1), 1), (0, full), (0x7F8, hi), (1 << 11, 0x7F8), (0x3F8 | 1 << 11, 0), (1 << 10, 0),
                         (0, 5), (3 << (n - 2), 3 << (n - 2))]
        # wider than a tile (as test_gpu_expectation._terms), tile passes between them
        out["wide"] = [(full, 0), (1 << 3, 1 << 3), (full, full), (full ^ 0b111, 0b101), (0, 1 << (n - 1)), ((full >> 3) << 3, 1 << (n - 1)),
                       (full & ~1, (1 << (n - 1)) | 1), (0x7FF, 0x7FF)]
    return out


def _apply_and_compare(c, psi, pairs, rng, what):
    x = np.array([p[0] for p in pairs], dtype=np.uint64)
    z = np.array([p[1] for p in pairs], dtype=np.uint64)
    th = rng.uniform(-np.pi, np.pi, len(pairs))
    assert len(pairs) <= 128
    c.upload(psi)
    passes = c.apply_pauli_rotations(x, z, th)
    got = c.download()
    err = float(np.max(np.abs(got - rotate_list(psi, x, z, th))))
    print(f"{what}: {len(pairs)} rotations in {passes} passes, max |got - want| = {err:.3e} (bound {ATOL:g})")
    assert err < ATOL, (what, err)
    assert passes == c.last_rotation_passes == len(plan_pauli_rotations(c.k, x)[1]), what
    return passes


@pytest.mark.parametrize("n", list(range(1, 15)))
def test_against_the_reference(n):
    psi = _rand_state(n, n)
    rng = np.random.default_rng(500 + n)
    c = DeviceChunk.empty(n)
    try:
        passes = {name: _apply_and_compare(c, psi, pairs, rng, f"n={n} {name}") for name, pairs in _lists(n, 100 + n).items()}
        if n >= 12:
            assert passes["breaks"] >= 5 and passes["wide"] >= 8 and passes["z_outside"] == 1, passes
        else:
            assert set(passes.values()) == {1}, passes       # the whole chunk is one tile
        c.upload(psi)
        assert c.apply_pauli_rotations([], [], []) == 0      # nothing launched
        assert np.array_equal(c.download(), psi)
    finally:
        c.close()


def test_rotations_are_applied_in_list_order():
    n, q = 12, 5
    full = (1 << n) - 1
    psi = _rand_state(n, 40)
    X, Z = (1 << q, 0), (0, 1 << q)
    cases = {
        "one pass": ([X, Z], 1),                                          # X on q, then Z on q, from the same tile
        "across a wide pass": ([X, (full, 0), Z], 3),                     # tile, wide, tile
        "across a tile break": ([(0x7F8, 0), (1 << 11, 1 << q)], 2),      # X on 3..10, then X on 11 with Z on q: 12 bits
    }
    c = DeviceChunk.empty(n)
    try:
        for name, (pairs, passes) in cases.items():
            x = np.array([p[0] for p in pairs], dtype=np.uint64)
            z = np.array([p[1] for p in pairs], dtype=np.uint64)
            th = np.array([0.7, 0.9, -0.6][:len(pairs)])
            c.upload(psi)
            assert c.apply_pauli_rotations(x, z, th) == passes, name
            got = c.download()
            forward, backward = rotate_list(psi, x, z, th), rotate_list(psi, x[::-1], z[::-1], th[::-1])
            assert float(np.max(np.abs(got - forward))) < ATOL, name
            assert float(np.max(np.abs(got - backward))) > 1e-3, name
    finally:
        c.close()


def test_more_rotations_than_a_pass_holds():
    """1030 rotations inside one 11-bit tile of a 13-qubit state (four tiles): the planner splits the list at 1024, so the
    second pass reads the term table at an offset of 1024 entries; then 1530 such rotations with a wide rotation at
    position 500: three tile passes and one wide pass (500, 1, 1024, 6 rotations; table offsets 500, 501 and 1525), the
    split at 1024 behind a wide pass.  Every amplitude against the reference at ATOL:
    tests/test_pauli_rotation_cpu.py shows that the reference's own rounding over the longer list and back stays below
    1e-13, so the bound tests the kernel."""
    psi = _rand_state(LONG_N, 61)
    x, z, th = long_rotation_list()
    pass_of, tiles = plan_pauli_rotations(LONG_N, x)
    assert [int(v) for v in np.bincount(pass_of)] == [1024, 6] and int(tiles[0]) == LONG_TILE and 0 not in [int(t) for t in tiles]
    assert np.count_nonzero(x == 0) > 300 and np.count_nonzero(z & np.uint64(0b1001000)) > 500
    full = (1 << LONG_N) - 1
    xw, zw, thw = long_rotation_list(1530, seed=62)
    xw, zw, thw = np.insert(xw, 500, np.uint64(full)), np.insert(zw, 500, np.uint64(0b1001001)), np.insert(thw, 500, 0.45)
    pass_w, tiles_w = plan_pauli_rotations(LONG_N, xw)
    assert [int(v) for v in np.bincount(pass_w)] == [500, 1, 1024, 6]
    assert [int(t) != 0 for t in tiles_w] == [True, False, True, True]
    c = DeviceChunk.empty(LONG_N)
    try:
        for what, (xs, zs, ts), passes in (("one tile", (x, z, th), 2), ("with a wide rotation", (xw, zw, thw), 4)):
            c.upload(psi)
            assert c.apply_pauli_rotations(xs, zs, ts) == passes == c.last_rotation_passes, what
            got = c.download()
            err = float(np.max(np.abs(got - rotate_list(psi, xs, zs, ts))))
            print(f"{what}: {len(xs)} rotations in {passes} passes, max |got - want| = {err:.3e} (bound {ATOL:g})")
            assert err < ATOL, (what, err)
            assert float(np.max(np.abs(got - rotate_list(psi, xs[::-1], zs[::-1], ts[::-1])))) > 1e-3, what
    finally:
        c.close()


def test_inverse_norm_and_repeatability():
    n = 13
    psi = _rand_state(n, 41)
    rng = np.random.default_rng(42)
    lists = _lists(n, 43)
    pairs = lists["weights"] + lists["wide"] + lists["breaks"] + lists["z_outside"]
    x = np.array([p[0] for p in pairs], dtype=np.uint64)
    z = np.array([p[1] for p in pairs], dtype=np.uint64)
    th = rng.uniform(-np.pi, np.pi, len(pairs))
    c = DeviceChunk.from_numpy(psi)
    try:
        c.apply_pauli_rotations(x, z, th)
        first = c.download()
        assert abs(c.norm2() - 1.0) < 1e-13
        c.apply_pauli_rotations(x[::-1], z[::-1], -th[::-1])
        back = float(np.max(np.abs(c.download() - psi)))
        print(f"theta then -theta over {len(pairs)} rotations: max |after - before| = {back:.3e} (bound 1e-13)")
        assert back < 1e-13
        assert float(np.max(np.abs(first - psi))) > 1e-3
        c.upload(psi)
        c.apply_pauli_rotations(x, z, th)
        assert c.download().tobytes() == first.tobytes()                  # the same bits from the same start
    finally:
        c.close()


def test_against_the_gate_path():
    n = 12
    psi = _rand_state(n, 44)
    c = DeviceChunk.empty(n)
    try:
        for label, theta in (("Z0 Z1", 0.37), ("X2 Y5", -1.1)):
            x, z, theta = evolution.rotation(label, theta)
            c.upload(psi)
            c.apply_ops(rotation_gates(x, z, theta))
            want = c.download()
            c.upload(psi)
            c.apply_pauli_rotations([x], [z], [theta])
            got = c.download()
            assert float(np.max(np.abs(got - want))) < ATOL, label
            assert float(np.max(np.abs(got - psi))) > 1e-3, label
    finally:
        c.close()


def test_views():
    psi = _rand_state(14, 45)
    lists = _lists(10, 46)
    pairs = lists["singles"] + lists["weights"] + lists["top"]
    x = np.array([p[0] for p in pairs], dtype=np.uint64)
    z = np.array([p[1] for p in pairs], dtype=np.uint64)
    th = np.random.default_rng(47).uniform(-np.pi, np.pi, len(pairs))
    assert len(pairs) <= 128
    c = DeviceChunk.empty(14)
    try:
        for off in (0, 3 << 10, 15 << 10):
            c.upload(psi)
            v = c.view(off, 10)
            try:
                assert v.apply_pauli_rotations(x, z, th) == 1
            finally:
                v.close()
            got = c.download()
            assert float(np.max(np.abs(got[off:off + 1024] - rotate_list(psi[off:off + 1024], x, z, th)))) < ATOL, off
            outside = np.ones(1 << 14, dtype=bool)
            outside[off:off + 1024] = False
            assert got[outside].tobytes() == psi[outside].tobytes(), off      # the parent outside the view: bitwise unchanged
    finally:
        c.close()


def test_grid_stride_loop_at_22_qubits():
    """2^22 amplitudes: 2048 tiles, two per workgroup under the cap of 1024 workgroups (64 MiB: the cached instantiation)."""
    n = 22
    full = (1 << n) - 1
    psi = _rand_state(n, 48)
    pairs = [(1 << 3, 0), (0, 1 << 21), (0x18, 0x10 | 1 << 21), (1 << 21, 1 << 20), (3 << 12, 1 << 12), (full, 5 << 19), (0, 0),
             (0x7F8, full), (1 << 10 | 1 << 20, 1 << 21), (0, full)]
    x = np.array([p[0] for p in pairs], dtype=np.uint64)
    z = np.array([p[1] for p in pairs], dtype=np.uint64)
    th = np.random.default_rng(49).uniform(-np.pi, np.pi, len(pairs))
    tiles = plan_pauli_rotations(n, x)[1]
    assert 0 in [int(t) for t in tiles] and len(tiles) == 4          # tile, wide, tile, tile
    c = DeviceChunk.from_numpy(psi)
    try:
        assert c.apply_pauli_rotations(x, z, th) == len(tiles)
        err = float(np.max(np.abs(c.download() - rotate_list(psi, x, z, th))))
        print(f"n=22: {len(pairs)} rotations in {len(tiles)} passes, max |got - want| = {err:.3e} (bound {ATOL:g})")
        assert err < ATOL
    finally:
        c.close()


def test_streaming_instantiation():
    """A 12-qubit view inside a 2^25 allocation (512 MiB, more than the 256 MiB Infinity Cache): the non-temporal forms of
    k_rot_tile and k_rot_wide.  Only the view and the 2^12 amplitudes on either side are uploaded and downloaded."""
    n, w = 12, 1 << 12
    off = 1234 * w
    window = _rand_state(n + 2, 50)[:3 * w]                     # left guard | view | right guard
    psi = window[w:2 * w]
    lists = _lists(n, 51)
    pairs = lists["weights"] + lists["wide"] + lists["breaks"] + lists["z_outside"]
    x = np.array([p[0] for p in pairs], dtype=np.uint64)
    z = np.array([p[1] for p in pairs], dtype=np.uint64)
    th = np.random.default_rng(52).uniform(-np.pi, np.pi, len(pairs))
    assert len(pairs) <= 128
    parent = DeviceChunk.empty(25)
    view = parent.view(off, n)
    try:
        parent.upload(window, offset=off - w)
        view.profile_begin()
        passes = view.apply_pauli_rotations(x, z, th)
        entry = [e for e in view.profile_end() if e["kernel"].startswith("k_rot")]
        assert len(entry) == 1 and entry[0]["launches"] == passes and entry[0]["streaming_launches"] == passes, entry
        assert entry[0]["algorithmic_bytes"] == entry[0]["hbm_bytes"] == 32.0 * w * passes
        got = parent.download(off - w, 3 * w)
        assert float(np.max(np.abs(got[w:2 * w] - rotate_list(psi, x, z, th)))) < ATOL
        assert got[:w].tobytes() == window[:w].tobytes() and got[2 * w:].tobytes() == window[2 * w:].tobytes()
    finally:
        view.close()
        parent.close()


def test_errors():
    from tests.test_gpu_kernels import _random_ops
    k = 14
    psi = _rand_state(k, 53)
    lib = _lib.load()
    c, buf = DeviceChunk.from_numpy(psi), DeviceChunk.empty(k)
    try:
        def call(x, z, th, n=None, passes=True, handle=c._h):
            xs, zs, ts = (None if a is None else np.array(a, dtype=t) for a, t in ((x, np.uint64), (z, np.uint64), (th, np.float64)))
            out = C.c_int(-1)
            return lib.qsim_apply_pauli_rotations(handle, 2 if n is None else n, _lib.ptr(xs), _lib.ptr(zs), _lib.ptr(ts),
                                                  C.byref(out) if passes else None)
        ok = ([1, 2], [0, 4], [0.1, 0.2])
        for xm, zm in ((1 << k, 0), (0, 1 << (k + 1)), (1, 1 << 63)):
            assert call([1, xm], [0, zm], [0.1, 0.2]) == _lib.QSIM_ERR_NONLOCAL
        for bad in (float("nan"), float("inf"), -float("inf")):
            assert call(ok[0], ok[1], [0.1, bad]) == _lib.QSIM_ERR_INVALID
        assert call(None, ok[1], ok[2]) == _lib.QSIM_ERR_INVALID
        assert call(ok[0], None, ok[2]) == _lib.QSIM_ERR_INVALID
        assert call(ok[0], ok[1], None) == _lib.QSIM_ERR_INVALID
        assert call(*ok, passes=False) == _lib.QSIM_ERR_INVALID
        assert call(*ok, handle=None) == _lib.QSIM_ERR_INVALID
        assert call(*ok, n=-1) == _lib.QSIM_ERR_INVALID
        assert call(None, None, None, n=0) == _lib.QSIM_OK
        with pytest.raises(NotImplementedError):
            c.apply_pauli_rotations([1 << k], [0], [0.1])
        with pytest.raises(ValueError):
            c.apply_pauli_rotations([1], [0], [float("nan")])
        with pytest.raises(ValueError):
            c.apply_pauli_rotations([1, 2], [0], [0.1])
        assert c.download().tobytes() == psi.tobytes()          # a refused call changes nothing
        # a split qsim_apply_ops_io has left pieces pending on the chunk: refused like a plain op list
        c.apply_ops_io(_random_ops(k, 10, 1), dst=(buf, [5], None, -1), parts=-2)
        assert c.pending_parts()
        with pytest.raises(ValueError, match="pending"):
            c.apply_pauli_rotations(*ok)
        for j in range(len(c.pending_parts())):
            c.store_part(j)
        assert call(*ok) == _lib.QSIM_OK
    finally:
        c.close()
        buf.close()


# ---- the engine and the runner -------------------------------------------------------------------------------------------
def _hamiltonian(n, seed):
    rng = np.random.default_rng(seed)
    terms = [(float(rng.uniform(0.5, 1.5)), {q: p, q + 1: p}) for q in range(n - 1) for p in "XYZ"]
    terms += [(0.4, {}), (0.3, {0: "Z", n - 1: "Y"}), (-0.6, {q: "X" for q in range(n)})]
    return PauliSum(terms, n_qubits=n)


@pytest.mark.parametrize("staged", [False, True], ids=["identity", "staged"])
def test_engine_evolve(staged):
    from quantum_simulations_amd.runner.engine import SingleGpuEngine
    n = 12
    eng = SingleGpuEngine(n, layout="search" if staged else "identity")
    try:
        eng.init_zero_state()
        eng.execute(eng.plan(gen.random_1q_cx_circuit(n, depth=6, seed=9), repeats=8 if staged else 1))
        if staged:
            l2p = [int(p) for p in np.random.default_rng(3).permutation(n)]
            eng._adopt_layout(l2p)                                   # (SWAP passes: the state now lives in that layout)
            assert eng.l2p == l2p
        else:
            assert eng.l2p is None or eng.l2p == list(range(n))
        H = _hamiltonian(n, 4)
        psi = eng.state_vector()
        layout = eng.l2p
        for order, steps in ((1, 2), (2, 1)):
            passes = eng.evolve(H, 0.3, steps=steps, order=order)
            psi = rotate_list(psi, *evolution.trotter_rotations(H, 0.3, steps, order))
            assert passes == eng.state.last_rotation_passes >= 1
        assert eng.l2p == layout and not eng._zero                  # the state did not move
        assert float(np.max(np.abs(eng.state_vector() - psi))) < ATOL
        eng.apply_pauli_rotations([("X0 Z3", 0.2), ({5: "Y"}, -0.4), (1 << 11, 1 << 11, 0.9)])
        psi = rotate_list(psi, [1, 1 << 5, 1 << 11], [1 << 3, 1 << 5, 1 << 11], [0.2, -0.4, 0.9])
        assert float(np.max(np.abs(eng.state_vector() - psi))) < ATOL
        # a single-term H commutes with its own evolution, which is exact: the energy is unchanged
        one = PauliSum({"X1 Y4 Z10": 0.8}, n_qubits=n)
        before = eng.expectation(one)
        eng.evolve(one, 1.7, steps=3, order=2)
        assert abs(eng.expectation(one) - before) < ATOL
        assert float(np.max(np.abs(eng.state_vector() - rotate_list(psi, [0b10010], [1 << 10 | 1 << 4], [0.8 * 1.7])))) < ATOL
    finally:
        eng.close()


@pytest.mark.parametrize("staged", [False, True], ids=["identity", "staged"])
def test_single_node_evolve(staged):
    from quantum_simulations_amd.runner import single_node
    n = 12
    cd = gen.random_1q_cx_circuit(n, depth=8, seed=5)
    buf = single_node.run(cd, chunk_size=1 << 9, use_fusion=True, use_staging=staged)
    try:
        l2p = getattr(buf, "log_to_phys", None) or None
        if staged:
            assert l2p and l2p != list(range(n))
        else:
            assert l2p is None or l2p == list(range(n))
        logical = (lambda v: v) if l2p is None else (lambda v: permute_state(v, l2p))
        psi = logical(buf.state.download())
        H = _hamiltonian(n, 7)
        passes = single_node.evolve(buf, H, 0.25, steps=2, order=2)
        assert passes == buf.state.last_rotation_passes >= 1
        want = rotate_list(psi, *evolution.trotter_rotations(H, 0.25, 2, 2))
        assert float(np.max(np.abs(logical(buf.state.download()) - want))) < ATOL
        assert float(np.max(np.abs(want - psi))) > 1e-3
    finally:
        buf.close()
