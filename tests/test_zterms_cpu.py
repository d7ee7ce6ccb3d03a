"""No GPU: the host side of the per-term Z expectations -- `diagonal.term_values`, `diagonal.correlations`, the flags of
`readout.expectation` and the cut of a long list in `DeviceChunk.expectation_z_terms` -- on the stand-in chunk of
tests/zterm_reference.py, which answers from the direct numpy sum and records its calls."""
import ctypes as C

import numpy as np
import pytest

from quantum_simulations_amd import _lib, diagonal, readout
from quantum_simulations_amd.kernel import device
from quantum_simulations_amd.kernel.device import DeviceChunk
from quantum_simulations_amd.observable import PauliSum, pauli_terms_np
from tests import zterm_reference as ref

N = 6
L2P = [4, 0, 5, 2, 1, 3]


def _rand_state(n, seed):
    rng = np.random.default_rng(seed)
    psi = rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)
    return psi / np.linalg.norm(psi)


def _in_layout(psi, l2p):
    """The state with logical qubit q on index bit l2p[q]."""
    i = np.arange(psi.size)
    j = np.zeros_like(i)
    for q, p in enumerate(l2p):
        j |= ((i >> q) & 1) << p
    out = np.empty_like(psi)
    out[j] = psi
    return out


PSI = _rand_state(N, 7) * 1.3                       # not normalised: the per-term values are not divided by norm2
D = PauliSum([(0.9, {0: "Z"}), (-0.4, {1: "Z", 2: "Z"}), (0.2, {}), (0.5, {0: "Z", 5: "Z"}), (0.7, {3: "Z"}), (-1.1, {2: "Z", 1: "Z", 4: "Z"})],
             n_qubits=N)
MIXED = PauliSum([(0.7, {0: "X", 1: "Z"}), (0.9, {0: "Z"}), (-0.3, {2: "Y"}), (0.5, {0: "Z", 3: "Z"}), (0.2, {1: "X", 3: "X"}),
                  (0.4, {}), (-0.6, {0: "Y", 1: "Y"}), (0.8, {2: "Z", 4: "Z", 5: "Z"})], n_qubits=N)


# ---- diagonal.term_values ------------------------------------------------------------------------------------------------
def test_term_values_are_in_term_order_without_coefficients():
    c = ref.HostZChunk(PSI)
    got = diagonal.term_values(c, None, D)
    assert c.calls == [("expectation_z_terms", len(D))]
    assert np.array_equal(c.z_masks[0], np.array(D.z, dtype=np.uint64))          # the sum's own order, nothing merged
    assert np.array_equal(got, ref.z_term_values(PSI, D.z))
    assert got[2] == ref.z_term_values(PSI, [0])[0] and abs(got[2] - 1.69) < 1e-12   # the identity: sum |psi|^2


def test_term_values_do_not_merge_what_diagonal_part_merges():
    # diagonal_part adds the coefficients of equal masks; the values keep one entry per term of the sum
    c = ref.HostZChunk(PSI)
    assert diagonal.term_values(c, None, D).shape == (len(D),) == diagonal.diagonal_part(D)[0].shape
    assert c.z_masks[0].size == len(D)


def test_term_values_put_the_layout_into_the_masks():
    c = ref.HostZChunk(_in_layout(PSI, L2P))
    got = diagonal.term_values(c, L2P, D)
    want_masks = [sum(1 << L2P[q] for q in range(N) if (z >> q) & 1) for z in D.z]
    assert [int(m) for m in c.z_masks[0]] == want_masks
    assert np.max(np.abs(got - ref.z_term_values(PSI, D.z))) < 1e-14
    assert np.array_equal(c.psi, _in_layout(PSI, L2P))                           # the state did not move


def test_term_values_refuse_a_term_with_x_or_y():
    c = ref.HostZChunk(PSI)
    with pytest.raises(ValueError, match="term 0 .* is not diagonal"):
        diagonal.term_values(c, None, MIXED)
    assert c.calls == []


# ---- diagonal.correlations -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connected", [True, False])
@pytest.mark.parametrize("qubits", [None, [4, 1, 3]])
@pytest.mark.parametrize("l2p", [None, L2P])
def test_correlations_against_numpy(l2p, qubits, connected):
    c = ref.HostZChunk(PSI if l2p is None else _in_layout(PSI, l2p))
    z, zz = diagonal.correlations(c, l2p, qubits, connected)
    qs = list(range(N)) if qubits is None else qubits
    m = len(qs)
    assert c.calls == [("expectation_z_terms", 1 + m + m * (m - 1) // 2)]          # ONE call: identity, singles, pairs
    wz, wzz = ref.correlations_np(PSI, qs, connected)
    assert z.shape == (m,) and zz.shape == (m, m)
    assert np.max(np.abs(z - wz)) < 1e-13 and np.max(np.abs(zz - wzz)) < 1e-13
    assert np.array_equal(zz, zz.T)
    assert np.max(np.abs(np.diag(zz) - (1.0 - z * z if connected else 1.0))) < 1e-15


def test_correlations_default_is_connected_and_bad_qubits_are_refused():
    c = ref.HostZChunk(PSI)
    assert np.array_equal(diagonal.correlations(c, None)[1], diagonal.correlations(c, None, None, True)[1])
    for bad in ([0, 0], [N], [-1]):
        with pytest.raises(ValueError, match="correlations"):
            diagonal.correlations(c, None, bad)
    with pytest.raises(ValueError, match="sum"):
        diagonal.correlations(ref.HostZChunk(np.zeros(1 << N)), None)


# ---- readout.expectation -------------------------------------------------------------------------------------------------
def test_both_flags_off_is_chunk_expectation_and_nothing_else():
    c = ref.HostZChunk(_in_layout(PSI, L2P))
    got = readout.expectation(c, L2P, MIXED)
    assert c.calls == [("expectation", None)]
    assert got == ref.HostZChunk(_in_layout(PSI, L2P)).expectation(MIXED, l2p=L2P)
    assert readout.expectation(c, L2P, MIXED, False, False) == got and len(c.calls) == 2


@pytest.mark.parametrize("fuse", [False, True])
def test_per_term_values_come_in_term_order_across_mixed_terms(monkeypatch, fuse):
    monkeypatch.setattr(readout, "Z_TERMS_MIN", 1)
    c = ref.HostZChunk(_in_layout(PSI, L2P))
    got = readout.expectation(c, L2P, MIXED, per_term=True, fuse_diagonal=fuse)
    want = pauli_terms_np(PSI, MIXED.x, MIXED.z)
    assert got.shape == (len(MIXED),) and got.dtype == np.float64
    assert np.max(np.abs(got - want)) < 1e-13
    n_z = sum(1 for x in MIXED.x if not x)
    assert c.calls == ([("expectation_z_terms", n_z), ("expectation_pauli", len(MIXED) - n_z)] if fuse else [("expectation_pauli", len(MIXED))])
    assert abs(MIXED.value(got) - readout.expectation(c, L2P, MIXED)) < 1e-13


def test_fuse_diagonal_routes_from_the_threshold_on(monkeypatch):
    n_z = sum(1 for x in MIXED.x if not x)
    plain = readout.expectation(ref.HostZChunk(PSI), None, MIXED)
    for threshold, fused in ((n_z, True), (n_z + 1, False), (n_z - 1, True)):
        monkeypatch.setattr(readout, "Z_TERMS_MIN", threshold)
        c = ref.HostZChunk(PSI)
        got = readout.expectation(c, None, MIXED, fuse_diagonal=True)
        names = [name for name, _ in c.calls]
        assert names == (["expectation_z_terms", "expectation_pauli"] if fused else ["expectation_pauli"]), threshold
        assert abs(got - plain) < 1e-13
    # a sum of Z-only terms: the per-term call is not made at all
    monkeypatch.setattr(readout, "Z_TERMS_MIN", 1)
    c = ref.HostZChunk(PSI)
    assert abs(readout.expectation(c, None, D, fuse_diagonal=True) - readout.expectation(c, None, D)) < 1e-13
    assert c.calls[0] == ("expectation_z_terms", len(D)) and [n for n, _ in c.calls] == ["expectation_z_terms", "expectation"]


def test_the_committed_threshold_is_a_positive_count():
    assert isinstance(readout.Z_TERMS_MIN, int) and readout.Z_TERMS_MIN >= 1


# ---- DeviceChunk.expectation_z_terms: the cut of a long list, on a stand-in library -----------------------------------
class _Library:
    """`qsim_expectation_z_terms` answered from the transform of tests/zterm_reference.py; records the size of every call."""

    def __init__(self, psi):
        self.table, self.sizes = ref.all_z_values(psi), []

    def qsim_expectation_z_terms(self, handle, n_terms, z_masks, out, n_passes):
        assert 0 <= n_terms <= 16384
        self.sizes.append(n_terms)
        if n_terms:
            z = np.ctypeslib.as_array(C.cast(z_masks, C.POINTER(C.c_uint64)), shape=(n_terms,))
            res = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_double)), shape=(n_terms,))
            res[:] = self.table[z.astype(np.int64)]
        n_passes._obj.value = (n_terms + 2047) // 2048
        return 0

    def qsim_destroy(self, handle):
        return 0


def test_a_list_above_16384_terms_is_split(monkeypatch):
    n = 15
    psi = _rand_state(n, 3)
    lib = _Library(psi)
    some = np.array([0, 1, 5, 1 << 14, (1 << 15) - 1, 12345], dtype=np.uint64)
    assert np.max(np.abs(lib.table[some.astype(np.int64)] - ref.z_term_values(psi, some))) < 1e-14
    monkeypatch.setattr(_lib, "load", lambda: lib)
    c = DeviceChunk(1, n, 0)
    masks = np.arange(1, 16384 + 7 + 1, dtype=np.uint64)                         # 16391 distinct Z strings
    got = c.expectation_z_terms(masks)
    assert lib.sizes == [16384, 7] and device.Z_TERMS_PER_CALL == 16384
    assert c.last_z_terms_passes == 8 + 1
    assert np.array_equal(got, lib.table[1:16384 + 7 + 1])
    assert c.expectation_z_terms(masks[:16384]).size == 16384 and lib.sizes[2:] == [16384]
    assert c.expectation_z_terms([]).size == 0 and lib.sizes[3:] == [0] and c.last_z_terms_passes == 0
    # ... and through readout.expectation: 16391 Z-only terms, the sum within 1e-13 of the direct one
    lib.sizes.clear()
    co = np.random.default_rng(5).standard_normal(masks.size)
    co /= np.sum(np.abs(co))
    obs = PauliSum([(float(a), {q: "Z" for q in range(n) if (int(m) >> q) & 1}) for a, m in zip(co, masks)], n_qubits=n)
    got = readout.expectation(c, None, obs, fuse_diagonal=True)
    assert lib.sizes == [16384, 7]
    assert abs(got - float(np.dot(co, lib.table[1:16384 + 7 + 1]))) < 1e-13
    c._h = C.c_void_p()                                                          # (nothing to destroy)
