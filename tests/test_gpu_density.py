"""qsim_reduced_density_matrix on an MI355X against the numpy restatement rdm_reference.rdm_np at 1e-12 (normalised
states; the reference stays 500 times inside that): every chunk size around the tile boundary, qubit placements and
orders, views, the grid-stride loop, the streaming instantiation, argument errors, the engine and single_node paths in
non-identity layouts, closed forms.  Every result must be exactly Hermitian and bitwise repeatable."""
import numpy as np
import pytest

from quantum_simulations_amd import _lib, density
from quantum_simulations_amd import circuits as gen
from quantum_simulations_amd.circuit.staging import permute_state
from quantum_simulations_amd.kernel.device import DeviceChunk
from tests.rdm_reference import rand_state, rdm_np

pytestmark = pytest.mark.gpu

TOL = 1e-12


def _check(chunk, psi, qs, full=True):
    """One qubit list against rdm_np; returns the largest deviation."""
    got = chunk.reduced_density_matrix(qs)
    want = rdm_np(psi, qs)
    d = 1 << len(qs)
    assert got.shape == (d, d) and got.dtype == np.complex128
    err = float(np.max(np.abs(got - want)))
    print(f"n={chunk.k} qubits={list(qs)}: max |rho - rdm_np| = {err:.3e}")
    assert err < TOL, (chunk.k, qs, err)
    assert np.array_equal(got, got.conj().T), (chunk.k, qs)          # exactly Hermitian
    assert np.all(got.diagonal().imag == 0.0), (chunk.k, qs)
    if full:
        tr_err = abs(float(np.trace(got).real) - chunk.norm2())
        p_err = float(np.max(np.abs(got.diagonal().real - chunk.probabilities(qs))))
        print(f"    |trace - norm2| = {tr_err:.3e}, max |diagonal - probabilities| = {p_err:.3e}")
        assert tr_err < TOL and p_err < TOL, (chunk.k, qs, tr_err, p_err)
        again = chunk.reduced_density_matrix(qs)
        assert got.tobytes() == again.tobytes(), (chunk.k, qs)       # bitwise repeatable
    return err


@pytest.mark.parametrize("n", list(range(1, 14)))
def test_every_chunk_size_around_the_tile(n):
    """n = r (no environment), n < 3 (less than a line), n < 8 (fewer amplitudes than threads), n = 11 (one tile),
    n = 12 and 13 (two and four tiles); every r = 1..min(n, 6) on a random subset in random order."""
    psi = rand_state(n, 500 + n)
    rng = np.random.default_rng(600 + n)
    c = DeviceChunk.from_numpy(psi)
    try:
        worst = 0.0
        for r in range(1, min(n, 6) + 1):
            for _ in range(2):
                qs = [int(q) for q in rng.permutation(n)[:r]]
                worst = max(worst, _check(c, psi, qs))
        print(f"n={n}: worst {worst:.3e}")
    finally:
        c.close()


def _placements(n, r):
    out = {"top": list(range(n - r, n)), "above the line": list(range(3, 3 + r)),
           "spread with one line bit": [1] + [int(q) for q in np.linspace(4, n - 1, r - 1).round()] if r > 1 else [1]}
    if r <= 3:
        out["inside the line"] = list(range(r))
    return out


@pytest.fixture(scope="module")
def state14():
    psi = rand_state(14, 1400)
    c = DeviceChunk.from_numpy(psi)
    yield c, psi
    c.close()


@pytest.mark.parametrize("r", [1, 2, 3, 4, 5, 6])
def test_qubit_placement_and_order(state14, r):
    """n = 14: the qubits inside the line bits (r <= 3), on the top bits, just above the line, spread out with one line
    bit; each ascending, descending and shuffled, against rdm_np on the same order (a swapped bit <-> qubits[j] mapping
    shows as permuted rows and columns)."""
    c, psi = state14
    rng = np.random.default_rng(r)
    for name, qs in _placements(14, r).items():
        assert len(set(qs)) == r, (name, qs)
        orders = [sorted(qs), sorted(qs, reverse=True), [int(q) for q in rng.permutation(qs)]]
        for order in orders:
            _check(c, psi, order)
        if r > 1:                                                    # and the permutation itself, on the device's results
            a, b = c.reduced_density_matrix(orders[0]), c.reduced_density_matrix(orders[1])
            idx = [int(f"{m:0{r}b}"[::-1], 2) for m in range(1 << r)]   # reversing the list reverses the bits of an index
            assert np.max(np.abs(a - b[np.ix_(idx, idx)])) < TOL, name


def test_views(state14):
    c, psi = state14
    rng = np.random.default_rng(7)
    for off in (0, 3 << 10, 15 << 10):
        v = c.view(off, 10)
        try:
            for r in range(1, 7):
                _check(v, psi[off: off + 1024], [int(q) for q in rng.permutation(10)[:r]])
        finally:
            v.close()


# the loop case: shared by the three tests below (23 qubits, 128 MiB; the references are computed once)
_LOOP_SETS = {1: [[22], [1]], 3: [[2, 22, 9]], 6: [[2, 9, 0, 22, 15, 5], [17, 18, 19, 20, 21, 16]]}


@pytest.fixture(scope="module")
def loop_state():
    psi = rand_state(23, 2323)
    return psi, {tuple(qs): rdm_np(psi, qs) for sets in _LOOP_SETS.values() for qs in sets}


@pytest.mark.parametrize("r", [1, 3, 6])
def test_a_workgroup_walks_four_tiles(loop_state, r):
    """The grid-stride loop of k_rdm_small (r = 1, 3) and k_rdm_mfma (r = 6).  A tile has kRdmTileBits = 11 bits
    whatever r is, and a launch has at most kRdmMaxWg = 1024 workgroups for every r (csrc/rdm_kernels.h), so a chunk of
    n qubits has 2^(n - 11) tiles and a workgroup walks 2^(n - 11 - 10) of them: n = 23 is the smallest size with at least
    three (four) tiles per workgroup -- n = 22 gives two.  Whoever changes either constant moves n with it.  The qubit
    sets include one with line bits and the top bit, [2, 9, 0, 22, 15, 5], where the outer bits have holes."""
    psi, want = loop_state
    c = DeviceChunk.from_numpy(psi)
    try:
        for qs in _LOOP_SETS[r]:
            got = c.reduced_density_matrix(qs)
            err = float(np.max(np.abs(got - want[tuple(qs)])))
            print(f"n=23 qubits={qs}: max |rho - rdm_np| = {err:.3e}")
            assert err < TOL, (qs, err)
            assert np.array_equal(got, got.conj().T) and np.all(got.diagonal().imag == 0.0)
            assert abs(float(np.trace(got).real) - c.norm2()) < TOL
            assert float(np.max(np.abs(got.diagonal().real - c.probabilities(qs)))) < TOL
            assert got.tobytes() == c.reduced_density_matrix(qs).tobytes()
    finally:
        c.close()


def _rdm_entries(chunk):
    return [e for e in chunk.profile_end() if e["kernel"].startswith("k_rdm")]


def test_the_streaming_instantiation(loop_state):
    """A 2^22 view at a nonzero offset inside a 2^25 parent (512 MiB > the 256 MiB Infinity Cache) takes the
    non-temporal instantiation -- two tiles per workgroup -- and a stand-alone 22-qubit chunk (64 MiB) the cached one."""
    psi = loop_state[0][: 1 << 22]
    psi = psi / np.linalg.norm(psi)
    sets = [[21], [2, 21, 9], [2, 9, 0, 21, 15, 5]]
    want = [rdm_np(psi, qs) for qs in sets]
    parent = DeviceChunk.empty(25)
    view = parent.view(5 << 22, 22)
    alone = DeviceChunk.from_numpy(psi)
    try:
        view.upload(psi)
        for chunk, streaming in ((view, 1), (alone, 0)):
            for qs, w in zip(sets, want):
                chunk.profile_begin()
                got = chunk.reduced_density_matrix(qs)
                entry = _rdm_entries(chunk)
                assert len(entry) == 1 and entry[0]["launches"] == 1 and entry[0]["streaming_launches"] == streaming, entry
                assert entry[0]["algorithmic_bytes"] == 16.0 * (1 << 22)
                err = float(np.max(np.abs(got - w)))
                print(f"streaming={streaming} qubits={qs}: max |rho - rdm_np| = {err:.3e}")
                assert err < TOL
                assert np.array_equal(got, got.conj().T) and np.all(got.diagonal().imag == 0.0)
        # the two instantiations sum in the same order
        assert view.reduced_density_matrix(sets[2]).tobytes() == alone.reduced_density_matrix(sets[2]).tobytes()
    finally:
        view.close()
        alone.close()
        parent.close()


def test_argument_errors():
    from tests.test_gpu_kernels import _random_ops
    k = 14
    c = DeviceChunk.from_numpy(rand_state(k, 3))
    buf = DeviceChunk.empty(k)
    try:
        lib = _lib.load()
        q = np.arange(8, dtype=np.int32)
        out = np.zeros(2 * 4 ** 6)
        qp, op = _lib.ptr(q), _lib.ptr(out)
        assert lib.qsim_reduced_density_matrix(c._h, 0, qp, op) == _lib.QSIM_ERR_INVALID
        assert lib.qsim_reduced_density_matrix(c._h, 7, qp, op) == _lib.QSIM_ERR_INVALID
        assert lib.qsim_reduced_density_matrix(c._h, 2, None, op) == _lib.QSIM_ERR_INVALID
        assert lib.qsim_reduced_density_matrix(c._h, 2, qp, None) == _lib.QSIM_ERR_INVALID
        assert lib.qsim_reduced_density_matrix(None, 2, qp, op) == _lib.QSIM_ERR_INVALID
        rep = np.array([3, 5, 3], dtype=np.int32)
        assert lib.qsim_reduced_density_matrix(c._h, 3, _lib.ptr(rep), op) == _lib.QSIM_ERR_INVALID
        far = np.array([1, k], dtype=np.int32)
        assert lib.qsim_reduced_density_matrix(c._h, 2, _lib.ptr(far), op) == _lib.QSIM_ERR_NONLOCAL
        neg = np.array([-1], dtype=np.int32)
        assert lib.qsim_reduced_density_matrix(c._h, 1, _lib.ptr(neg), op) != _lib.QSIM_OK
        assert lib.qsim_reduced_density_matrix(c._h, 6, qp, op) == _lib.QSIM_OK
        with pytest.raises(ValueError):
            c.reduced_density_matrix([])
        with pytest.raises(ValueError):
            c.reduced_density_matrix(list(range(7)))
        with pytest.raises(ValueError, match="repeated"):
            c.reduced_density_matrix([4, 4])
        with pytest.raises(NotImplementedError, match="non-local"):
            c.reduced_density_matrix([0, k])
        # slab pieces of a split call pending on the chunk: refused, and fine again once they are stored
        c.apply_ops_io(_random_ops(k, 10, 1), dst=(buf, [5], None, -1), parts=-2)
        with pytest.raises(ValueError, match="pending"):
            c.reduced_density_matrix([0, 1])
        for j in range(len(c.pending_parts())):
            c.store_part(j)
        assert c.reduced_density_matrix([0, 1]).shape == (4, 4)
    finally:
        c.close()
        buf.close()


def test_engine_in_a_non_identity_layout():
    from quantum_simulations_amd.runner.engine import SingleGpuEngine
    n = 14
    eng = SingleGpuEngine(n, layout="search")
    try:
        cd = gen.random_1q_cx_circuit(n, depth=6, seed=9)
        eng.init_zero_state()
        eng.execute(eng.plan(cd, repeats=8))
        l2p = [int(p) for p in np.random.default_rng(3).permutation(n)]
        eng._adopt_layout(l2p)                                   # (SWAP passes: the state now lives in that layout)
        assert eng.l2p is not None and eng.l2p != list(range(n))
        psi = eng.state_vector()
        before = eng.state.download()
        rng = np.random.default_rng(11)
        for r in range(1, 7):
            qs = [int(q) for q in rng.permutation(n)[:r]]
            got = eng.reduced_density_matrix(qs)
            err = float(np.max(np.abs(got - rdm_np(psi, qs))))
            print(f"engine qubits={qs}: max |rho - rdm_np| = {err:.3e}")
            assert err < TOL, (qs, err)
        assert np.array_equal(eng.state.download(), before)      # read-only
    finally:
        eng.close()


def test_single_node_staged():
    from quantum_simulations_amd.runner import single_node
    n = 12
    cd = gen.random_1q_cx_circuit(n, depth=8, seed=5)
    buf = single_node.run(cd, chunk_size=1 << 9, use_fusion=True, use_staging=True)
    try:
        assert buf.log_to_phys and buf.log_to_phys != list(range(n))
        psi = permute_state(single_node.collect_state(buf), buf.log_to_phys)   # the state in logical qubit order
        rng = np.random.default_rng(12)
        for r in range(1, 7):
            qs = [int(q) for q in rng.permutation(n)[:r]]
            got = single_node.reduced_density_matrix(buf, qs)
            err = float(np.max(np.abs(got - rdm_np(psi, qs))))
            print(f"single_node qubits={qs}: max |rho - rdm_np| = {err:.3e}")
            assert err < TOL, (qs, err)
    finally:
        buf.close()


def test_ghz_20_qubits():
    from quantum_simulations_amd.runner.engine import SingleGpuEngine
    n = 20
    eng = SingleGpuEngine(n)
    try:
        eng.init_zero_state()
        eng.execute(eng.plan(gen.generate_ghz_circuit(n)))
        worst = 0.0
        for q in range(n):
            rho = eng.reduced_density_matrix([q])
            worst = max(worst, float(np.max(np.abs(rho - np.eye(2) / 2))))
            assert abs(density.entropy(rho) - 1.0) < 1e-12, q
        print(f"GHZ 20: max |rho_q - I/2| = {worst:.3e}")
        assert worst < TOL
        rho = eng.reduced_density_matrix([0, 7, 19, 3, 12, 5])
        assert abs(density.purity(rho) - 0.5) < TOL and abs(density.entropy(rho) - 1.0) < 1e-12
    finally:
        eng.close()


def test_bell_pairs_entropy_counts_the_cut_pairs():
    """Ten Bell pairs on qubits (2i, 2i + 1): the entropy of a subset is the number of pairs it cuts.  Six qubits cut an
    even number of pairs (2 whole pairs + 2 cut, ...), so next to the 6-qubit subsets cutting 0, 2, 4 and 6 pairs the
    odd count, 3, is a 5-qubit subset (one whole pair and three cut)."""
    from quantum_simulations_amd.runner.engine import SingleGpuEngine
    n = 20
    gates = []
    for i in range(10):
        gates.append({"qubits": [2 * i], "gate": "H", "params": {}})
        gates.append({"qubits": [2 * i, 2 * i + 1], "gate": "CNOT", "params": {}})
    eng = SingleGpuEngine(n)
    try:
        eng.init_zero_state()
        eng.execute(eng.plan({"number_of_qubits": n, "gates": gates}))
        for qs, cut in (([0, 1, 6, 7, 18, 19], 0), ([2, 3, 9, 12, 14], 3), ([0, 19, 5, 8, 13, 2], 6),
                        ([2, 3, 9, 10, 11, 14], 2), ([16, 4, 5, 1, 9, 12], 4)):
            rho = eng.reduced_density_matrix(qs)
            s = density.entropy(rho)
            print(f"Bell pairs, qubits={qs}: entropy {s!r} (cuts {cut}), purity {density.purity(rho)!r}")
            assert abs(s - cut) < 1e-12, (qs, s)
            assert abs(density.purity(rho) - 2.0 ** -cut) < TOL
    finally:
        eng.close()
