"""The readout workspace of a chunk on an MI355X: probabilities, reduced density matrices, Pauli-sum expectation values
and shot sampling lay their partials out in ONE grown-on-demand device buffer per chunk (ensure_work,
csrc/readout_kernels.h).  Calls of different kinds interleaved on one chunk -- growing the buffer, then reusing it --
must give the bits of the same call on a fresh chunk (the kernels add in a fixed order: two calls give the same bits,
so the comparison is exact); a view owns a workspace of its own; a chunk is destroyed with its workspace allocated; and
the logical-layout wrappers (readout.py) give what SingleGpuEngine and single_node give."""
import numpy as np
import pytest

from quantum_simulations_amd import circuits as gen
from quantum_simulations_amd import readout, sampling
from quantum_simulations_amd.kernel.device import DeviceChunk
from quantum_simulations_amd.observable import PauliSum
from tests.pauli_reference import pauli_terms_operator
from tests.rdm_reference import rand_state, rdm_np
from tests.test_gpu_loop_paths import _probabilities_longdouble

pytestmark = pytest.mark.gpu

TOL = 1e-12


def _terms_in_one_tile(n, count, seed):
    """`count` strings whose X/Y lie on bits 0..10 (one tile pass of up to kExpMaxTerms = 1024 terms), Z anywhere."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 1 << min(n, 11), size=count).astype(np.uint64)
    z = rng.integers(0, 1 << n, size=count).astype(np.uint64)
    return x, z


def _calls(n):
    """The readout calls of the interleaved test, in order: (name, function of a chunk)."""
    x, z = _terms_in_one_tile(n, 600, 1)
    few, many = sampling.draw(10, 2), sampling.draw(200_000, 3)
    p8, r2, r6 = [0, 13, 5, 9, 2, 11, 7, 12], [12, 1], [3, 13, 0, 8, 10, 6]
    return [
        ("probabilities r=8", lambda c: c.probabilities(p8)),                 # 4 MiB + 2 KiB of partial histograms
        ("rdm r=2", lambda c: c.reduced_density_matrix(r2)),
        ("600 terms", lambda c: c.expectation_pauli(x, z)),                   # 1024 x 600 x 8 B of rows: the buffer grows
        ("10 shots", lambda c: c.sample(few)),
        ("200000 shots", lambda c: c.sample(many)),                           # 4.0 MB of slots: fits, no growth
        ("rdm r=6", lambda c: c.reduced_density_matrix(r6)),
        ("probabilities r=8 again", lambda c: c.probabilities(p8)),
        ("600 terms again", lambda c: c.expectation_pauli(x, z)),
    ], (p8, r2, r6, x, z)


def _fresh(psi, fn):
    c = DeviceChunk.from_numpy(psi)
    try:
        return fn(c)
    finally:
        c.close()


def test_interleaved_calls_on_one_chunk():
    n = 14
    psi = rand_state(n, 1414)
    calls, (p8, r2, r6, x, z) = _calls(n)
    c = DeviceChunk.from_numpy(psi)
    try:
        got = [fn(c) for _, fn in calls]
    finally:
        c.close()                                                             # (qsim_destroy with the workspace allocated)
    for (name, fn), g in zip(calls, got):
        assert g.tobytes() == _fresh(psi, fn).tobytes(), name
    assert got[6].tobytes() == got[0].tobytes() and got[7].tobytes() == got[2].tobytes()
    # one call of each kind against its host reference
    p = psi.real.astype(np.longdouble) ** 2 + psi.imag.astype(np.longdouble) ** 2
    want = _probabilities_longdouble(p, p8).astype(np.float64)
    np.testing.assert_allclose(got[6], want, rtol=TOL, atol=1e-15 * want.max())
    for g, qs in ((got[1], r2), (got[5], r6)):
        err = float(np.max(np.abs(g - rdm_np(psi, qs))))
        print(f"rdm qubits={qs}: max |rho - rdm_np| = {err:.3e}")
        assert err < TOL, (qs, err)
    err = float(np.max(np.abs(got[7] - pauli_terms_operator(psi, x, z))))
    print(f"600 terms: max |device - operator reference| = {err:.3e}")
    assert err < TOL, err
    # and another chunk after the first is gone
    d = DeviceChunk.from_numpy(psi)
    try:
        assert d.probabilities(p8).tobytes() == got[0].tobytes()
        assert d.sample(sampling.draw(10, 2)).tobytes() == got[3].tobytes()
    finally:
        d.close()


def test_a_view_owns_its_workspace():
    """A 12-qubit view and its 15-qubit parent read alternately: the view (600 terms), the parent (probabilities), the
    view (a density matrix); each against a fresh chunk of the same amplitudes."""
    psi = rand_state(15, 1515)
    off = 5 << 12
    x, z = _terms_in_one_tile(12, 600, 4)
    p8, r3 = [14, 0, 3, 12, 8, 1, 10, 6], [11, 2, 7]
    parent = DeviceChunk.from_numpy(psi)
    try:
        view = parent.view(off, 12)
        try:
            a = view.expectation_pauli(x, z)
            b = parent.probabilities(p8)
            c = view.reduced_density_matrix(r3)
        finally:
            view.close()
        again = parent.probabilities(p8)                                      # (the parent's buffer outlives the view)
    finally:
        parent.close()
    part = psi[off: off + (1 << 12)]
    assert a.tobytes() == _fresh(part, lambda f: f.expectation_pauli(x, z)).tobytes()
    assert b.tobytes() == _fresh(psi, lambda f: f.probabilities(p8)).tobytes() == again.tobytes()
    assert c.tobytes() == _fresh(part, lambda f: f.reduced_density_matrix(r3)).tobytes()
    assert float(np.max(np.abs(c - rdm_np(part, r3)))) < TOL


def _obs(n):
    rng = np.random.default_rng(8)
    terms = {}
    while len(terms) < 12:
        qs = rng.choice(n, size=int(rng.integers(1, 4)), replace=False)
        terms[" ".join(f"{'XYZ'[int(rng.integers(3))]}{int(q)}" for q in sorted(qs))] = float(rng.standard_normal())
    return PauliSum(terms, n_qubits=n)


def test_the_layout_wrappers_once():
    """12 qubits in a non-identity layout: SingleGpuEngine.* and single_node.* are the readout.* calls on (chunk, l2p)."""
    from quantum_simulations_amd.runner import single_node
    from quantum_simulations_amd.runner.engine import SingleGpuEngine
    n = 12
    cd = gen.random_1q_cx_circuit(n, depth=8, seed=5)
    obs, qs = _obs(n), [7, 0, 10, 3]
    results = {}
    eng = SingleGpuEngine(n, layout="search")
    try:
        eng.init_zero_state()
        eng.execute(eng.plan(cd, repeats=8))
        eng._adopt_layout([int(p) for p in np.random.default_rng(3).permutation(n)])
        assert eng.l2p is not None and eng.l2p != list(range(n))
        results["engine"] = (eng.expectation(obs), eng.reduced_density_matrix(qs), eng.sample(2003, seed=4), eng.sample(2003, seed=4, qubits=qs))
        results["engine, direct"] = (readout.expectation(eng.state, eng.l2p, obs), readout.reduced_density_matrix(eng.state, eng.l2p, qs),
                                     readout.sample(eng.state, eng.l2p, 2003, 4), readout.sample(eng.state, eng.l2p, 2003, 4, qs))
    finally:
        eng.close()
    buf = single_node.run(cd, chunk_size=1 << 9, use_fusion=True, use_staging=True)
    try:
        assert buf.log_to_phys and buf.log_to_phys != list(range(n))
        results["single_node"] = (single_node.expectation(buf, obs), single_node.reduced_density_matrix(buf, qs),
                                  single_node.sample(buf, 2003, seed=4), single_node.sample(buf, 2003, seed=4, qubits=qs))
        results["single_node, direct"] = (readout.expectation(buf.state, buf.log_to_phys, obs), readout.reduced_density_matrix(buf.state, buf.log_to_phys, qs),
                                          readout.sample(buf.state, buf.log_to_phys, 2003, 4), readout.sample(buf.state, buf.log_to_phys, 2003, 4, qs))
    finally:
        buf.close()
    for who in ("engine", "single_node"):
        (e, rho, idx, marg), (e2, rho2, idx2, marg2) = results[who], results[who + ", direct"]
        assert e == e2 and rho.tobytes() == rho2.tobytes() and np.array_equal(idx, idx2) and np.array_equal(marg, marg2), who
        assert np.array_equal(marg, sampling.marginal(idx, qs)), who
    # the two routes hold the same logical state up to rounding
    assert abs(results["engine"][0] - results["single_node"][0]) < TOL
    assert float(np.max(np.abs(results["engine"][1] - results["single_node"][1]))) < TOL
