"""qsim_expectation_z_terms on an MI355X against the direct sum of tests/zterm_reference.

Bound.  A value is a sum of non-negative weights of total norm2 = 1 with signs.  On the device it passes through 11
add/sub stages, a sequential sum over a workgroup's at most 2^(k-21) tiles and the sum over at most 1024 rows: at most
(11 + 2^(k-21) + 1024) eps <= 1.7e-13 at k = 30, so the project's 1e-12 absolute holds at every size.  A host model of
the tiled algorithm against exact sums (tools/diag_plan_check.cpp, k = 1 .. 16) stays below 2e-16, numpy's pairwise direct
sum of the reference carries about log2(2^n) eps: the reference is four orders inside the bound."""
import ctypes as C

import numpy as np
import pytest

from quantum_simulations_amd import _lib, diagonal, readout
from quantum_simulations_amd import circuits as gen
from quantum_simulations_amd.circuit.staging import permute_state
from quantum_simulations_amd.kernel.device import DeviceChunk
from quantum_simulations_amd.observable import PauliSum
from tests import zterm_reference as ref

pytestmark = pytest.mark.gpu

ATOL = 1e-12
KERNEL = "k_diag_term_values per-term Z expectations"
PASS_TERMS = 2048        # terms one pass serves (kDiagValuesPerPass)


def _rand_state(n, seed):
    rng = np.random.default_rng(seed)
    psi = rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)
    return psi / np.linalg.norm(psi)


def _subset(rng, bits, w):
    m = 0
    for b in rng.choice(bits, size=w, replace=False):
        m |= 1 << int(b)
    return m


def _families(n, seed):
    rng = np.random.default_rng(seed)
    lo_bits, hi_bits = list(range(min(n, 11))), list(range(11, n))
    out = {"singles": [1 << q for q in range(n)],
           "pairs": [(1 << a) | (1 << b) for a in range(n) for b in range(a + 1, n)] or [1],
           "identity": [0],
           "full": [(1 << n) - 1],
           "low": [_subset(rng, lo_bits, int(rng.integers(1, len(lo_bits) + 1))) for _ in range(30)],
           "weights": [_subset(rng, n, 1 + i % n) for i in range(64)]}
    if hi_bits:
        out["high"] = [_subset(rng, hi_bits, int(rng.integers(1, len(hi_bits) + 1))) for _ in range(20)]
    dup = [_subset(rng, n, 1 + i % n) for i in range(5)]
    out["duplicates"] = dup + dup[::-1] + dup[:2] + [0, 0]
    return {k: np.array(v, dtype=np.uint64) for k, v in out.items()}


@pytest.mark.parametrize("n", range(1, 15))
def test_every_family_against_the_direct_sum(n):
    """n = 1 .. 10: a chunk smaller than a tile; 11: exactly one tile; 12 .. 14: outer-sign bits."""
    psi = _rand_state(n, 100 + n)
    rng = np.random.default_rng(n)
    c = DeviceChunk.from_numpy(psi)
    try:
        norm2 = c.norm2()
        for name, z in _families(n, 200 + n).items():
            got = c.expectation_z_terms(z)
            assert got.dtype == np.float64 and got.shape == z.shape
            assert c.last_z_terms_passes == 1
            err = float(np.max(np.abs(got - ref.z_term_values(psi, z))))
            print(f"n = {n:2d} {name:10s} {z.size:3d} terms: max |got - direct| = {err:.3e} (bound {ATOL:.0e})")
            assert err < ATOL, (n, name)
            assert c.expectation_z_terms(z).tobytes() == got.tobytes(), (n, name)          # a fixed summation order
            for t in np.nonzero(z == 0)[0]:
                assert abs(got[t] - norm2) < 1e-13, (n, name)
            if name == "duplicates":
                assert got[:5].tobytes() == got[9:4:-1].tobytes() and got[:2].tobytes() == got[10:12].tobytes()
            co = rng.standard_normal(z.size)
            m1 = c.diagonal_moments(z, co)[1]
            assert abs(float(np.dot(co, got)) - m1) < ATOL * float(np.sum(np.abs(co))), (n, name)
            assert float(np.max(np.abs(got - c.expectation_pauli(np.zeros_like(z), z)))) < ATOL, (n, name)
        assert c.download().tobytes() == psi.tobytes()                                   # read-only
    finally:
        c.close()


@pytest.mark.parametrize("count", [PASS_TERMS + 1, PASS_TERMS - 1, PASS_TERMS])
def test_pass_boundaries(count):
    n = 12
    psi = _rand_state(n, 31)
    z = np.random.default_rng(count).integers(0, 1 << n, size=count, dtype=np.uint64)
    c = DeviceChunk.from_numpy(psi)
    try:
        c.profile_begin()
        got = c.expectation_z_terms(z)
        entry = [e for e in c.profile_end() if e["kernel"] == KERNEL]
        passes = 2 if count > PASS_TERMS else 1
        assert c.last_z_terms_passes == passes
        assert len(entry) == 1 and entry[0]["launches"] == passes and entry[0]["streaming_launches"] == 0, entry
        assert entry[0]["algorithmic_bytes"] == entry[0]["hbm_bytes"] == 16.0 * (1 << n) * passes
        want = ref.z_term_values(psi, z)
        assert float(np.max(np.abs(got - want))) < ATOL
        assert abs(got[-1] - want[-1]) < ATOL and abs(got[PASS_TERMS - 2] - want[PASS_TERMS - 2]) < ATOL   # both sides of the boundary
        assert c.expectation_z_terms(z).tobytes() == got.tobytes()
        assert c.download().tobytes() == psi.tobytes()
    finally:
        c.close()


def test_no_terms_launch_nothing():
    psi = _rand_state(12, 5)
    lib = _lib.load()
    c = DeviceChunk.from_numpy(psi)
    try:
        c.profile_begin()
        got = c.expectation_z_terms([])
        assert c.profile_end() == []
        assert got.shape == (0,) and got.dtype == np.float64 and c.last_z_terms_passes == 0
        passes = C.c_int(7)
        assert lib.qsim_expectation_z_terms(c._h, 0, None, None, C.byref(passes)) == _lib.QSIM_OK and passes.value == 0
        assert lib.qsim_expectation_z_terms(c._h, 0, None, None, None) == _lib.QSIM_OK
    finally:
        c.close()


def test_errors():
    from tests.test_gpu_kernels import _random_ops
    k = 14
    psi = _rand_state(k, 82)
    lib = _lib.load()
    c, buf = DeviceChunk.from_numpy(psi), DeviceChunk.empty(k)
    try:
        def call(z, n=None, handle=c._h, out=True, passes=True):
            zs = None if z is None else np.array(z, dtype=np.uint64)
            res = np.zeros(max(len(z) if z is not None else 1, 1))
            return lib.qsim_expectation_z_terms(handle, (len(z) if n is None else n), _lib.ptr(zs), _lib.ptr(res) if out else None,
                                                C.byref(C.c_int(0)) if passes else None)

        for zm in (1 << k, 1 << (k + 1), 1 << 63):
            assert call([1, zm]) == _lib.QSIM_ERR_NONLOCAL
        assert b"term 1 acts on index bit" in lib.qsim_last_error() and b"log2(chunk_size)=14" in lib.qsim_last_error()
        assert call([1] * 16385) == _lib.QSIM_ERR_INVALID                      # 16385 terms through the raw ABI
        assert b"16385 terms in one call, at most 16384" in lib.qsim_last_error()
        assert call([1] * 16384) == _lib.QSIM_OK
        assert call([1, 6], n=-1) == _lib.QSIM_ERR_INVALID
        assert call(None, n=2) == _lib.QSIM_ERR_INVALID
        assert call([1, 6], out=False) == _lib.QSIM_ERR_INVALID
        assert call([1, 6], handle=None) == _lib.QSIM_ERR_INVALID
        assert call([1, 6], passes=False) == _lib.QSIM_OK                      # n_passes may be null
        with pytest.raises(NotImplementedError):
            c.expectation_z_terms([1 << k])
        assert c.download().tobytes() == psi.tobytes()
        # a split qsim_apply_ops_io has left pieces pending on the chunk: refused like the other diagonal calls
        c.apply_ops_io(_random_ops(k, 10, 1), dst=(buf, [5], None, -1), parts=-2)
        assert c.pending_parts()
        with pytest.raises(ValueError, match="pending"):
            c.expectation_z_terms([1, 6])
        for j in range(len(c.pending_parts())):
            c.store_part(j)
        assert call([1, 6]) == _lib.QSIM_OK
    finally:
        c.close()
        buf.close()


def _product_state(n, seed):
    """|0..0> with one RY(theta_q) per qubit, made on the device: <Z^z> = prod_{q in z} cos(theta_q)."""
    theta = np.random.default_rng(seed).uniform(0.3, 2.8, size=n)
    ops = [([q], np.array([[np.cos(t / 2), -np.sin(t / 2)], [np.sin(t / 2), np.cos(t / 2)]], dtype=np.complex128)) for q, t in enumerate(theta)]
    c = DeviceChunk.zero_state(n)
    c.apply_ops(ops)
    return c, np.cos(theta)


def _product_values(cos, z):
    return np.array([np.prod([cos[q] for q in range(cos.size) if (int(m) >> q) & 1]) for m in z])


def test_grid_stride_loop_at_22_qubits():
    """2^11 tiles on 1024 workgroups: every workgroup adds two tiles."""
    n = 22
    c, cos = _product_state(n, 22)
    try:
        rng = np.random.default_rng(1)
        z = np.array([1 << q for q in range(n)] + [(1 << a) | (1 << b) for a in range(n) for b in range(a + 1, n)]
                     + [int(m) for m in rng.integers(1, 1 << n, size=50)], dtype=np.uint64)
        got = c.expectation_z_terms(z)
        err = float(np.max(np.abs(got - _product_values(cos, z))))
        print(f"n = 22, {z.size} terms on the product state: max |got - prod cos| = {err:.3e} (bound {ATOL:.0e})")
        assert err < ATOL and c.last_z_terms_passes == 1
        assert c.expectation_z_terms(z).tobytes() == got.tobytes()
    finally:
        c.close()


def test_streaming_form_at_25_qubits():
    """512 MiB: above the 256 MiB from which the non-temporal instantiation runs."""
    n = 25
    c, cos = _product_state(n, 25)
    try:
        pairs = [(a, b) for a in range(0, 11) for b in range(11, n)][3::7][:20]          # every pair straddles bit 11
        assert len(pairs) == 20
        z = np.array([1 << q for q in range(n)] + [(1 << a) | (1 << b) for a, b in pairs], dtype=np.uint64)
        c.profile_begin()
        got = c.expectation_z_terms(z)
        entry = [e for e in c.profile_end() if e["kernel"] == KERNEL]
        assert len(entry) == 1 and entry[0]["launches"] == entry[0]["streaming_launches"] == 1, entry
        err = float(np.max(np.abs(got - _product_values(cos, z))))
        print(f"n = 25, {z.size} terms on the product state: max |got - prod cos| = {err:.3e} (bound {ATOL:.0e})")
        assert err < ATOL
    finally:
        c.close()


def test_correlations_of_ghz_and_under_a_layout_of_single_node(monkeypatch):
    from quantum_simulations_amd.runner import single_node
    n = 12
    ghz = np.zeros(1 << n, dtype=np.complex128)
    ghz[0] = ghz[-1] = np.sqrt(0.5)
    c = DeviceChunk.from_numpy(ghz)
    try:
        z, zz = diagonal.correlations(c, None, connected=False)
        assert float(np.max(np.abs(z))) < ATOL and float(np.max(np.abs(zz - 1.0))) < ATOL
        z, zz = diagonal.correlations(c, None)
        assert float(np.max(np.abs(zz - 1.0))) < ATOL                                    # connected: z = 0 changes nothing
        sub = diagonal.correlations(c, None, [7, 2, 11], connected=False)[1]
        assert sub.shape == (3, 3) and float(np.max(np.abs(sub - 1.0))) < ATOL
    finally:
        c.close()
    # the GHZ circuit through the runner, in whatever layout it leaves the state
    buf = single_node.run(gen.generate_ghz_circuit(n), chunk_size=1 << 9, use_fusion=True, use_staging=True)
    try:
        z, zz = diagonal.correlations(buf.state, buf.l2p, connected=False)
        assert float(np.max(np.abs(z))) < ATOL and float(np.max(np.abs(zz - 1.0))) < ATOL
    finally:
        buf.close()
    # a random circuit that the runner leaves in a non-identity layout: against numpy on the logical state
    buf = single_node.run(gen.random_1q_cx_circuit(n, depth=8, seed=5), chunk_size=1 << 9, use_fusion=True, use_staging=True)
    try:
        l2p = buf.l2p
        assert l2p and list(l2p) != list(range(n))
        psi = permute_state(buf.state.download(), l2p)
        for qubits, connected in ((None, True), ([9, 0, 4, 11], False)):
            z, zz = diagonal.correlations(buf.state, l2p, qubits, connected)
            wz, wzz = ref.correlations_np(psi, list(range(n)) if qubits is None else qubits, connected)
            assert float(np.max(np.abs(z - wz))) < ATOL and float(np.max(np.abs(zz - wzz))) < ATOL
        monkeypatch.setattr(readout, "Z_TERMS_MIN", 1)                                  # 13 Z-only terms take the fused route
        obs = PauliSum([(0.5, {q: "Z", (q + 1) % n: "Z"}) for q in range(n)] + [(-1.5, {q: "X"}) for q in range(n)] + [(0.25, {})], n_qubits=n)
        plain = single_node.expectation(buf, obs)
        per_term = single_node.expectation(buf, obs, True, True)
        assert per_term.shape == (len(obs),) and abs(obs.value(per_term) - plain) < ATOL * float(np.sum(np.abs(obs.coeffs)))
        assert abs(single_node.expectation(buf, obs, fuse_diagonal=True) - plain) < ATOL * float(np.sum(np.abs(obs.coeffs)))
        values = diagonal.term_values(buf.state, l2p, PauliSum([(1.0, {q: "Z"}) for q in range(n)], n_qubits=n))
        assert float(np.max(np.abs(values - ref.z_term_values(psi, [1 << q for q in range(n)])))) < ATOL
    finally:
        buf.close()
