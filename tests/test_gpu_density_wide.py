"""qsim_reduced_density_matrix_wide (7 to 12 qubits, 64 x 64 blocks on the matrix cores) on an MI355X against the numpy
restatement rdm_reference.rdm_np at the 1e-12 of tests/test_gpu_density.py (normalised states; at r >= 7 the sums are
shorter than in the cases in which that reference stayed 500 times inside the bound): chunk sizes around the tile,
placements and orders, the r <= 6 call, views, the slice loop, the streaming instantiation, the errors, and the physics
of `density.subsystem` / `schmidt_spectrum` / `entanglement_entropy` / `entropy_profile` through the engine and
single_node.  Every result must be exactly Hermitian with a real diagonal, have the trace norm2, come out bitwise equal
a second time and leave the state's bytes alone."""
import numpy as np
import pytest

from quantum_simulations_amd import _lib, density
from quantum_simulations_amd import circuits as gen
from quantum_simulations_amd.circuit.staging import permute_state
from quantum_simulations_amd.kernel.device import DeviceChunk
from tests.rdm_reference import rand_state, rdm_np

pytestmark = pytest.mark.gpu

TOL = 1e-12
KERNEL = "k_rdm_wide density matrix of 7 to 12 qubits"


def _check(chunk, psi, qs, want=None, again=True):
    """One qubit list against rdm_np and the properties every result has; returns the matrix."""
    got = chunk.reduced_density_matrix_wide(qs)
    want = rdm_np(psi, qs) if want is None else want
    d = 1 << len(qs)
    assert got.shape == (d, d) and got.dtype == np.complex128
    err = float(np.max(np.abs(got - want)))
    tr_err = abs(float(np.trace(got).real) - chunk.norm2())
    print(f"n={chunk.k} qubits={list(qs)}: max |rho - rdm_np| = {err:.3e}, |trace - norm2| = {tr_err:.3e} (bound {TOL:.0e})")
    assert err < TOL, (chunk.k, qs, err)
    assert np.array_equal(got, got.conj().T), (chunk.k, qs)          # exactly Hermitian
    assert np.all(got.diagonal().imag == 0.0), (chunk.k, qs)
    assert tr_err < TOL, (chunk.k, qs, tr_err)
    if again:
        assert got.tobytes() == chunk.reduced_density_matrix_wide(qs).tobytes(), (chunk.k, qs)   # bitwise repeatable
    return got


def _profiled(chunk, psi, qs, want=None):
    """`_check` of one call under the launch profile; the profile is closed also when the check fails."""
    chunk.profile_begin()
    try:
        got = _check(chunk, psi, qs, want=want, again=False)
    finally:
        entries = chunk.profile_end()
    return got, entries


def _sizes(r):
    """n = r (no environment), r + 1, r + 2, the n at which the tile first has all its 11 bits (the r - 6 block
    qubits lie outside it: n = r + 5, which is 15 for r = 10), and 14 for r <= 10; only r = 11 and 12 stay at n <= 14
    (their first full tile would be n = 16 and 17)."""
    ns = {r, r + 1, r + 2}
    if r <= 10:
        ns |= {r + 5, 14}
    return sorted(n for n in ns if r <= 10 or n <= 14)


@pytest.mark.parametrize("r,n", [(r, n) for r in range(7, 13) for n in _sizes(r)])
def test_chunk_sizes_around_the_tile(r, n):
    psi = rand_state(n, 7000 + 100 * r + n)
    rng = np.random.default_rng(100 * r + n)
    c = DeviceChunk.from_numpy(psi)
    try:
        before = c.download().tobytes()
        qs = [int(q) for q in rng.permutation(n)[:r]]
        _check(c, psi, qs)
        assert c.download().tobytes() == before                      # read-only
    finally:
        c.close()


@pytest.fixture(scope="module")
def state14():
    psi = rand_state(14, 1414)
    c = DeviceChunk.from_numpy(psi)
    yield c, psi
    c.close()


def _placements(n, r):
    """The last set is the one whose block qubits (the selected qubits on the highest physical bits) come first in the
    caller's list, below the row qubits in the index of the result: the output map has to undo the split."""
    top = list(range(n - r, n))
    return {"all three line bits": list(range(r)), "top": top, "no line bit": list(range(3, 3 + r)),
            "spread with one line bit": [1] + [int(q) for q in np.linspace(4, n - 1, r - 1).round()],
            "block qubits first": top[::-1][: r - 6] + [0, 2] + list(range(4, 8))}


@pytest.mark.parametrize("r", [7, 8, 10])
def test_qubit_placement_and_order(state14, r):
    c, psi = state14
    rng = np.random.default_rng(r)
    before = c.download().tobytes()
    for name, qs in _placements(14, r).items():
        assert len(set(qs)) == r and len(qs) == r, (name, qs)
        if name == "spread with one line bit":
            assert sum(q < 3 for q in qs) == 1
        orders = [sorted(qs), sorted(qs, reverse=True), [int(q) for q in rng.permutation(qs)]]
        if name == "block qubits first":
            orders.append(qs)
        res = [_check(c, psi, order, again=(i == 0)) for i, order in enumerate(orders)]
        idx = [int(f"{m:0{r}b}"[::-1], 2) for m in range(1 << r)]   # reversing the list reverses the bits of an index
        assert np.max(np.abs(res[0] - res[1][np.ix_(idx, idx)])) < TOL, name
    assert c.download().tobytes() == before


def _trace_down(rho, r, keep):
    """Tr over the qubits of a (2^r, 2^r) matrix (bit j <-> list position j) whose positions are not in `keep`; bit i of
    the result <-> position keep[i]."""
    rest = [j for j in range(r) if j not in keep]
    rows = [r - 1 - j for j in reversed(keep)] + [r - 1 - j for j in reversed(rest)]
    t = rho.reshape([2] * (2 * r)).transpose(rows + [r + a for a in rows])
    d, e = 1 << len(keep), 1 << len(rest)
    return np.einsum("atbt->ab", t.reshape(d, e, d, e))


@pytest.mark.parametrize("r", [7, 9])
def test_consistent_with_the_narrow_call_and_probabilities(state14, r):
    c, psi = state14
    rng = np.random.default_rng(40 + r)
    qs = [int(q) for q in rng.permutation(14)[:r]]
    rho = c.reduced_density_matrix_wide(qs)
    keep = [int(j) for j in rng.permutation(r)[:6]]
    narrow = c.reduced_density_matrix([qs[j] for j in keep])
    err = float(np.max(np.abs(_trace_down(rho, r, keep) - narrow)))
    m = min(r, 8)
    keep8 = [int(j) for j in rng.permutation(r)[:m]]
    diag = _trace_down(np.diag(rho.diagonal()), r, keep8).diagonal().real
    p_err = float(np.max(np.abs(diag - c.probabilities([qs[j] for j in keep8]))))
    print(f"r={r} qubits={qs}: max |Tr_rest rho - narrow| = {err:.3e}, max |diagonal - probabilities| = {p_err:.3e} (bound {TOL:.0e})")
    assert err < TOL and p_err < TOL


@pytest.mark.parametrize("r", [7, 10])
def test_views(state14, r):
    c, psi = state14
    rng = np.random.default_rng(70 + r)
    for off in (3 << 10, 15 << 10):
        v = c.view(off, 10)
        try:
            _check(v, psi[off: off + 1024], [int(q) for q in rng.permutation(10)[:r]])
        finally:
            v.close()


# the slice loop: r -> (n, qubit sets); the references are computed once
_LOOP = {7: (23, [[2, 9, 0, 22, 15, 5, 11], [16, 17, 18, 19, 20, 21, 22]]), 8: (22, [[2, 9, 0, 21, 15, 5, 11, 18]])}


@pytest.fixture(scope="module")
def loop_state():
    return rand_state(23, 2323)


@pytest.mark.parametrize("r", [7, 8])
def test_a_workgroup_walks_four_tiles(loop_state, r):
    """A launch has pairs * S workgroups, S the largest power of two with pairs * S <= kRdmWideMaxWg = 2048
    (csrc/rdm_plan.h): S = 512 for the 3 pairs of r = 7, 128 for the 10 pairs of r = 8.  The outer index has
    n - 11 - (r - 6) bits (a tile has kRdmTileBits = 11, the block qubits are not walked), so a workgroup walks
    2^(n - 5 - r) / S outer tiles: n = 23 (r = 7) and n = 22 (r = 8) are the smallest sizes with at least three (four);
    one qubit less gives two.  Whoever changes either constant moves n with it.  The first set of each r has line bits
    and the top bit."""
    n, sets = _LOOP[r]
    psi = loop_state[: 1 << n]
    psi = psi / np.linalg.norm(psi)
    c = DeviceChunk.from_numpy(psi)
    try:
        for qs in sets:
            assert max(qs) == n - 1
            got, entries = _profiled(c, psi, qs)
            entries = [e for e in entries if e["kernel"].startswith("k_rdm")]
            assert len(entries) == 1 and entries[0]["kernel"] == KERNEL and entries[0]["launches"] == 1, entries
            assert entries[0]["algorithmic_bytes"] == float((1 << (r - 6)) * 16 * (1 << n)), entries
            assert got.tobytes() == c.reduced_density_matrix_wide(qs).tobytes()
    finally:
        c.close()


def test_the_streaming_instantiation(loop_state):
    """A 2^22 view at a nonzero offset inside a 2^25 parent (512 MiB > the 256 MiB Infinity Cache) takes the
    non-temporal instantiation, a stand-alone 22-qubit chunk (64 MiB) the cached one: both sum in the same order."""
    psi = loop_state[: 1 << 22]
    psi = psi / np.linalg.norm(psi)
    qs = [2, 21, 9, 0, 15, 5, 12]
    want = rdm_np(psi, qs)
    parent = DeviceChunk.empty(25)
    view = parent.view(5 << 22, 22)
    alone = DeviceChunk.from_numpy(psi)
    try:
        view.upload(psi)
        res = []
        for chunk, streaming in ((view, 1), (alone, 0)):
            got, entries = _profiled(chunk, psi, qs, want)
            res.append(got)
            entry = [e for e in entries if e["kernel"] == KERNEL]
            assert len(entry) == 1 and entry[0]["launches"] == 1 and entry[0]["streaming_launches"] == streaming, entry
            assert entry[0]["algorithmic_bytes"] == 2 * 16.0 * (1 << 22)
        assert res[0].tobytes() == res[1].tobytes()
    finally:
        view.close()
        alone.close()
        parent.close()


def test_argument_errors():
    from tests.test_gpu_kernels import _random_ops
    k = 14
    psi = rand_state(k, 3)
    c = DeviceChunk.from_numpy(psi)
    buf = DeviceChunk.empty(k)
    try:
        lib = _lib.load()
        q = np.arange(13, dtype=np.int32)
        out = np.zeros(2 * 4 ** 7)
        qp, op = _lib.ptr(q), _lib.ptr(out)
        wide = lib.qsim_reduced_density_matrix_wide
        for r in (0, 6, 13):
            assert wide(c._h, r, qp, op) == _lib.QSIM_ERR_INVALID
            assert b"qsim_reduced_density_matrix serves r <= 6" in lib.qsim_last_error()
        assert wide(c._h, 7, None, op) == _lib.QSIM_ERR_INVALID
        assert wide(c._h, 7, qp, None) == _lib.QSIM_ERR_INVALID
        assert wide(None, 7, qp, op) == _lib.QSIM_ERR_INVALID
        rep = np.array([3, 5, 0, 1, 2, 4, 3], dtype=np.int32)
        assert wide(c._h, 7, _lib.ptr(rep), op) == _lib.QSIM_ERR_INVALID
        assert b"repeated qubit 3" in lib.qsim_last_error()
        assert b"qsim_reduced_density_matrix_wide: repeated qubit 3" in lib.qsim_last_error()
        far = np.array([0, 1, 2, 3, 4, 5, k], dtype=np.int32)
        assert wide(c._h, 7, _lib.ptr(far), op) == _lib.QSIM_ERR_NONLOCAL
        neg = np.array([0, 1, 2, 3, 4, 5, -1], dtype=np.int32)
        assert wide(c._h, 7, _lib.ptr(neg), op) == _lib.QSIM_ERR_INVALID
        assert b"is negative" in lib.qsim_last_error()
        assert not out.any()                                         # nothing written by a refused call
        assert wide(c._h, 7, qp, op) == _lib.QSIM_OK
        with pytest.raises(ValueError, match="7 to 12"):
            c.reduced_density_matrix_wide(list(range(6)))
        with pytest.raises(ValueError, match="7 to 12"):
            c.reduced_density_matrix_wide(list(range(13)))
        with pytest.raises(ValueError, match="repeated"):
            c.reduced_density_matrix_wide([0, 1, 2, 3, 4, 5, 5])
        with pytest.raises(NotImplementedError, match="non-local"):
            c.reduced_density_matrix_wide([0, 1, 2, 3, 4, 5, k])
        assert np.array_equal(c.download(), psi)
        # slab pieces of a split call pending on the chunk: refused, and fine again once they are stored
        c.apply_ops_io(_random_ops(k, 10, 1), dst=(buf, [5], None, -1), parts=-2)
        with pytest.raises(ValueError, match="pending"):
            c.reduced_density_matrix_wide(list(range(7)))
        for j in range(len(c.pending_parts())):
            c.store_part(j)
        assert c.reduced_density_matrix_wide(list(range(7))).shape == (128, 128)
    finally:
        c.close()
        buf.close()


# ---- physics, through the engine in a non-identity layout and through single_node

# Entropies of matrices of up to 4096 x 4096 whose exact value is known only through eigvalsh: LAPACK bounds the error of
# an eigenvalue by about dim * eps * ||rho|| (4096 * 2.2e-16 = 9e-13), and an eigenvalue lam carries that into the entropy
# with the factor |log2 lam| + 1.44; the widest case below, 256 eigenvalues of 2^-8, gives 256 * 9.44 * 9e-13 = 2.2e-9 as
# the guaranteed bound.  Errors are far smaller in practice, and 1e-9 separates the integer counts all the same.  The GHZ
# cases and the spectrum against the SVD keep the 1e-12 the issue sets.
ENT_TOL = 1e-9


def _engine(n, cd, seed):
    from quantum_simulations_amd.runner.engine import SingleGpuEngine
    eng = SingleGpuEngine(n, layout="search")
    eng.init_zero_state()
    eng.execute(eng.plan(cd))
    eng._adopt_layout([int(p) for p in np.random.default_rng(seed).permutation(n)])   # (SWAP passes: the state now lives there)
    assert eng.l2p is not None and eng.l2p != list(range(n))
    return eng


def _staged(cd):
    from quantum_simulations_amd.runner import single_node
    return single_node.run(cd, chunk_size=1 << 12, use_fusion=True, use_staging=True)


def _bell_pairs(n):
    gates = []
    for i in range(n // 2):
        gates.append({"qubits": [2 * i], "gate": "H", "params": {}})
        gates.append({"qubits": [2 * i, 2 * i + 1], "gate": "CNOT", "params": {}})
    return {"number_of_qubits": n, "gates": gates}


@pytest.mark.parametrize("holder", ["engine", "single_node"])
def test_ghz_20_qubits_has_one_bit_across_every_cut(holder):
    """Cuts of 7, 10 and 13 qubits: 13 goes through the complement (7 qubits)."""
    n = 20
    cd = gen.generate_ghz_circuit(n)
    h = _engine(n, cd, 5) if holder == "engine" else _staged(cd)
    try:
        rng = np.random.default_rng(20)
        for m in (7, 10, 13):
            qs = [int(q) for q in rng.permutation(n)[:m]]
            s = density.entanglement_entropy(h.state, h.l2p, qs)
            s2 = density.entanglement_entropy(h.state, h.l2p, qs, alpha=2)
            print(f"GHZ 20 ({holder}), {m} qubits {qs}: S = {s!r}, S_2 = {s2!r}")
            assert abs(s - 1.0) < 1e-12 and abs(s2 - 1.0) < 1e-12, (qs, s, s2)
        lam = density.schmidt_spectrum(h.state, h.l2p, list(range(13)))
        assert lam.shape == (128,) and np.max(np.abs(lam[:2] - 0.5)) < 1e-12 and np.max(lam[2:]) < 1e-12
    finally:
        h.close()


@pytest.mark.parametrize("holder", ["engine", "single_node"])
def test_bell_pairs_entropy_counts_the_cut_pairs(holder):
    """Ten Bell pairs on qubits (2i, 2i + 1): the entropy of a subset is the number of pairs it cuts.  The bound ENT_TOL
    is explained at its definition."""
    n = 20
    cd = _bell_pairs(n)
    h = _engine(n, cd, 6) if holder == "engine" else _staged(cd)
    try:
        cases = (([0, 1, 2, 3, 4, 5, 6, 7], 0), ([0, 2, 4, 6, 8, 10, 12, 14], 8), ([19, 0, 1, 5, 8, 9, 12, 2], 4),
                 ([0, 1, 2, 3, 4, 6, 8, 10, 12, 14], 6), ([1, 3, 5, 7, 9, 11, 13, 15, 17, 19], 10),
                 ([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12], 2), ([0, 2, 4, 6, 8, 10, 12, 14, 16, 18, 1, 3], 8))
        for qs, cut in cases:
            assert len(qs) in (8, 10, 12)
            s = density.entanglement_entropy(h.state, h.l2p, qs)
            print(f"Bell pairs ({holder}), {len(qs)} qubits {qs}: entropy {s!r} (cuts {cut})")
            assert abs(s - cut) < ENT_TOL, (qs, s)
            assert abs(density.purity(density.subsystem(h.state, h.l2p, qs)) - 2.0 ** -cut) < TOL
    finally:
        h.close()


@pytest.mark.parametrize("holder", ["engine", "single_node"])
def test_schmidt_spectrum_and_profile_of_a_random_state(holder):
    """16 qubits across 8 | 8: the spectrum is the squared singular values of the reshaped state; the entropy profile is
    symmetric under reversing `order` (the cut m of one order is the cut n - m of the other: the same spectrum)."""
    from quantum_simulations_amd.runner import single_node
    n = 16
    cd = gen.random_1q_cx_circuit(n, depth=10, seed=16)
    h = _engine(n, cd, 7) if holder == "engine" else _staged(cd)
    try:
        if holder == "engine":
            psi = h.state_vector()
        else:
            psi = single_node.collect_state(h)
            psi = permute_state(psi, h.log_to_phys) if h.l2p is not None else psi
        psi = psi / np.linalg.norm(psi)
        a = [3, 0, 12, 7, 9, 14, 5, 10]
        rest = [q for q in range(n) if q not in a]
        m = psi.reshape([2] * n).transpose([n - 1 - q for q in reversed(a)] + [n - 1 - q for q in reversed(rest)]).reshape(256, 256)
        want = np.sort(np.linalg.svd(m, compute_uv=False) ** 2)[::-1]
        lam = density.schmidt_spectrum(h.state, h.l2p, a)
        err = float(np.max(np.abs(lam - want)))
        print(f"random 16 ({holder}): max |spectrum - svd^2| = {err:.3e} (bound 1e-12)")
        assert lam.shape == (256,) and np.all(np.diff(lam) <= 0) and err < 1e-12
        order = [int(q) for q in np.random.default_rng(8).permutation(n)]
        fwd = density.entropy_profile(h.state, h.l2p, order)
        bwd = density.entropy_profile(h.state, h.l2p, order[::-1])
        assert fwd.shape == (n - 1,) and not np.isnan(fwd).any()
        sym = float(np.max(np.abs(fwd - bwd[::-1])))
        print(f"    entropy profile {np.round(fwd, 4).tolist()}: max |S(m) - S'(n - m)| = {sym:.3e}")
        assert sym < ENT_TOL
        assert abs(fwd[7] - density.entanglement_entropy(h.state, h.l2p, order[:8])) == 0.0
    finally:
        h.close()
