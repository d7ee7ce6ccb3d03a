"""No GPU: the host side of the entanglement readout -- `density.subsystem`, `schmidt_spectrum`, `entanglement_entropy`
and `entropy_profile` on a numpy stand-in chunk that records which device call it received."""
import numpy as np
import pytest

from quantum_simulations_amd import density
from tests.rdm_reference import rand_state, rdm_np


class RecordingChunk:
    """The two matrix calls of a DeviceChunk over a host array of PHYSICAL amplitudes, with the r limits of each."""

    def __init__(self, psi):
        self.psi = np.asarray(psi, dtype=np.complex128)
        self.k = int(self.psi.size).bit_length() - 1
        self.calls = []

    def reduced_density_matrix(self, qubits):
        assert 1 <= len(qubits) <= 6
        self.calls.append(("narrow", [int(q) for q in qubits]))
        return rdm_np(self.psi, qubits)

    def reduced_density_matrix_wide(self, qubits):
        assert 7 <= len(qubits) <= 12
        self.calls.append(("wide", [int(q) for q in qubits]))
        return rdm_np(self.psi, qubits)


class CountingChunk:
    """A chunk of k bits that only counts: every matrix is the identity (entropy = the number of qubits asked for)."""

    def __init__(self, k):
        self.k = k
        self.calls = []

    def reduced_density_matrix(self, qubits):
        self.calls.append(("narrow", len(qubits)))
        return np.eye(1 << len(qubits), dtype=np.complex128)

    def reduced_density_matrix_wide(self, qubits):
        self.calls.append(("wide", len(qubits)))
        return np.eye(1 << len(qubits), dtype=np.complex128)


def _in_layout(psi_logical, l2p):
    """The physical amplitudes of a logical state in the layout l2p (logical qubit q on index bit l2p[q])."""
    n = len(l2p)
    phys = np.arange(1 << n)
    logical = np.zeros_like(phys)
    for q, p in enumerate(l2p):
        logical |= ((phys >> p) & 1) << q
    return psi_logical[logical]


def test_dispatch_at_6_7_12_13_qubits():
    psi = rand_state(14, 1)
    c = RecordingChunk(psi)
    for r, kind in ((1, "narrow"), (6, "narrow"), (7, "wide"), (12, "wide")):
        qs = list(range(13, 13 - r, -1))
        rho = density.subsystem(c, None, qs)
        assert c.calls[-1] == (kind, qs) and rho.shape == (1 << r, 1 << r)
    n_calls = len(c.calls)
    with pytest.raises(ValueError, match="1 to 12 qubits expected, got 13"):
        density.subsystem(c, None, list(range(13)))
    with pytest.raises(ValueError, match="1 to 12 qubits expected, got 0"):
        density.subsystem(c, None, [])
    with pytest.raises(ValueError, match="repeated qubit"):
        density.subsystem(c, None, [1, 2, 1])
    with pytest.raises(ValueError, match="outside 0..13"):
        density.subsystem(c, None, [1, 14])
    assert len(c.calls) == n_calls


def test_the_layout_goes_into_the_qubit_list():
    n = 10
    l2p = [int(p) for p in np.random.default_rng(2).permutation(n)]
    psi = rand_state(n, 2)
    c = RecordingChunk(_in_layout(psi, l2p))
    for qs in ([4, 0, 7], [9, 1, 2, 3, 8, 5, 0]):
        rho = density.subsystem(c, l2p, qs)
        assert c.calls[-1][1] == [l2p[q] for q in qs]
        assert np.max(np.abs(rho - rdm_np(psi, qs))) < 1e-14
    assert np.max(np.abs(density.subsystem(c, l2p, [4, 0, 7]) - rdm_np(c.psi, [4, 0, 7]))) > 1e-3   # (the layout matters)


def test_the_complement_is_taken_exactly_when_2a_exceeds_n():
    n = 10
    c = RecordingChunk(rand_state(n, 3))
    density.schmidt_spectrum(c, None, [7, 2, 9, 0, 4])                 # 2 |A| = n: A itself, in the caller's order
    assert c.calls[-1] == ("narrow", [7, 2, 9, 0, 4])
    density.schmidt_spectrum(c, None, [7, 2, 9, 0, 4, 5])              # 2 |A| > n: the complement, ascending
    assert c.calls[-1] == ("narrow", [1, 3, 6, 8])
    density.schmidt_spectrum(c, None, [8, 1, 3, 5, 6, 7, 9, 0, 2])     # 9 | 1
    assert c.calls[-1] == ("narrow", [4])
    l2p = [int(p) for p in np.random.default_rng(4).permutation(n)]
    density.schmidt_spectrum(c, l2p, [0, 1, 2, 3, 4, 5, 6])            # the complement in LOGICAL qubits, then the layout
    assert c.calls[-1] == ("narrow", [l2p[7], l2p[8], l2p[9]])
    c14 = RecordingChunk(rand_state(14, 5))
    density.schmidt_spectrum(c14, None, list(range(7)))
    assert c14.calls[-1] == ("wide", list(range(7)))


def test_value_error_texts():
    c = CountingChunk(30)
    with pytest.raises(ValueError, match=r"the cut 13 \| 17 has more than 12 qubits on both sides"):
        density.schmidt_spectrum(c, None, list(range(13)))
    with pytest.raises(ValueError, match=r"the cut 17 \| 13 has more than 12 qubits on both sides"):
        density.entanglement_entropy(c, None, list(range(17)))
    with pytest.raises(ValueError, match="1 to 29 of them on one side, got 30"):
        density.schmidt_spectrum(c, None, list(range(30)))
    with pytest.raises(ValueError, match="1 to 29 of them on one side, got 0"):
        density.schmidt_spectrum(c, None, [])
    with pytest.raises(ValueError, match="alpha = 0"):
        density.entanglement_entropy(c, None, [0], alpha=0)
    with pytest.raises(ValueError, match="permutation of 0..29"):
        density.entropy_profile(c, None, order=[0, 1])
    assert c.calls == []
    assert density.schmidt_spectrum(c, None, list(range(18))).shape == (4096,)   # 18 | 12: the complement
    assert c.calls == [("wide", 12)]


def test_renyi_2_is_minus_log2_purity_and_alpha_to_1_is_von_neumann():
    n = 10
    c = RecordingChunk(rand_state(n, 6))
    qs = [1, 8, 3, 6]
    rho = rdm_np(c.psi, qs)
    s2 = density.entanglement_entropy(c, None, qs, alpha=2)
    assert abs(s2 + np.log2(density.purity(rho))) < 1e-13
    s1 = density.entanglement_entropy(c, None, qs)
    assert abs(s1 - density.entropy(rho)) < 1e-13
    near = density.entanglement_entropy(c, None, qs, alpha=1 + 1e-6)
    assert abs(near - s1) < 1e-5 and near != s1
    assert density.entanglement_entropy(c, None, qs, alpha=0.5) > s1 > s2        # Renyi entropies decrease in alpha
    assert abs(density.entanglement_entropy(c, None, qs, base=np.e) - s1 * np.log(2)) < 1e-13


def test_nan_positions_of_the_profile_at_30_qubits():
    c = CountingChunk(30)
    prof = density.entropy_profile(c, None)
    assert prof.shape == (29,)
    m = np.arange(1, 30)
    assert np.array_equal(np.isnan(prof), np.minimum(m, 30 - m) > 12)            # cuts 13 .. 17
    # the identity matrix of the evaluated side: its entropy is that side's qubit count
    assert np.max(np.abs(prof[~np.isnan(prof)] - np.minimum(m, 30 - m)[~np.isnan(prof)])) < 1e-13
    assert len(c.calls) == 24 and c.calls[:7] == [("narrow", j) for j in range(1, 7)] + [("wide", 7)]
    assert [k for k, _ in c.calls].count("wide") == 12


def test_schmidt_spectrum_against_the_svd_at_10_qubits():
    n = 10
    psi = rand_state(n, 7)
    l2p = [int(p) for p in np.random.default_rng(8).permutation(n)]
    c = RecordingChunk(_in_layout(psi, l2p))
    for a in ([0, 1, 2, 3, 4], [9, 2, 5], [1, 2, 3, 4, 5, 6, 7], [3]):
        rest = [q for q in range(n) if q not in a]
        m = psi.reshape([2] * n).transpose([n - 1 - q for q in reversed(a)] + [n - 1 - q for q in reversed(rest)])
        sv = np.linalg.svd(m.reshape(1 << len(a), -1), compute_uv=False) ** 2
        lam = density.schmidt_spectrum(c, l2p, a)
        small = min(len(a), n - len(a))
        assert lam.shape == (1 << small,) and np.all(np.diff(lam) <= 0) and np.all(lam >= 0)
        assert np.max(np.abs(lam - np.sort(sv)[::-1][: 1 << small])) < 1e-14
        assert abs(lam.sum() - 1.0) < 1e-14
    prof = density.entropy_profile(c, l2p)
    back = density.entropy_profile(c, l2p, order=list(range(n - 1, -1, -1)))
    assert np.max(np.abs(prof - back[::-1])) < 1e-13


def test_the_older_functions_are_unchanged():
    rho = rdm_np(rand_state(8, 9), [1, 5, 2])
    lam = np.clip(np.linalg.eigvalsh(rho / np.trace(rho).real), 0, None)
    lam = lam[lam > 0]
    assert abs(density.entropy(rho) + np.sum(lam * np.log2(lam))) < 1e-14
    assert abs(density.purity(rho) - np.sum(lam ** 2)) < 1e-14
    assert "64 x 64" not in density.__doc__.split("\n")[0]
