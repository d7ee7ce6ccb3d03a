"""No GPU: the host references of tests/twostate_reference.py pinned against explicit Kronecker matrices (n <= 4) and
central differences, and quantum_simulations_amd.hamiltonian -- host bookkeeping over five chunk calls -- driven through
a numpy stand-in chunk that implements those calls from the references (precedent: tests/cpu_shard_backend.py)."""
import numpy as np
import pytest

from quantum_simulations_amd import hamiltonian
from quantum_simulations_amd.observable import PauliSum, as_pauli_sum
from tests.pauli_reference import apply_pauli
from tests.rotation_reference import rotate_list
from tests.twostate_reference import apply_sum, energy, gradient_forward, matrix_elements

_PAULI = {(0, 0): np.eye(2), (1, 0): np.array([[0, 1], [1, 0]]), (1, 1): np.array([[0, -1j], [1j, 0]]), (0, 1): np.diag([1.0, -1.0])}


def _rand_state(n, seed):
    rng = np.random.default_rng(seed)
    psi = rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)
    return psi / np.linalg.norm(psi)


def _kron(n, x, z):
    """The 2^n x 2^n matrix of a string, qubit q = bit q of the index (the highest qubit is the leftmost factor)."""
    m = np.eye(1, dtype=np.complex128)
    for q in reversed(range(n)):
        m = np.kron(m, _PAULI[((x >> q) & 1, (z >> q) & 1)])
    return m


def _random_sum(n, n_terms, seed):
    rng = np.random.default_rng(seed)
    xs = [int(v) for v in rng.integers(0, 1 << n, n_terms)]
    zs = [int(v) for v in rng.integers(0, 1 << n, n_terms)]
    co = rng.uniform(-1, 1, n_terms)
    return xs, zs, co / np.sum(np.abs(co))


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_references_against_kronecker_matrices(n):
    psi, phi = _rand_state(n, n), _rand_state(n, 10 + n)
    xs = [x for x in range(1 << n) for _ in range(1 << n)]
    zs = [z for _ in range(1 << n) for z in range(1 << n)]      # every string
    co = np.random.default_rng(n).uniform(-1, 1, len(xs))
    co /= np.sum(np.abs(co))
    mats = [_kron(n, x, z) for x, z in zip(xs, zs)]
    H = sum(c * m for c, m in zip(co, mats))
    assert np.max(np.abs(apply_sum(psi, xs, zs, co) - H @ psi)) < 1e-14
    want = np.array([np.vdot(phi, m @ psi) for m in mats])
    assert np.max(np.abs(matrix_elements(phi, psi, xs, zs) - want)) < 1e-14
    assert np.max(np.abs(matrix_elements(phi, psi, xs, zs) - np.conj(matrix_elements(psi, phi, xs, zs)))) < 1e-14


def test_gradient_forward_against_central_differences():
    n, n_rot, h = 4, 7, 1e-6
    rng = np.random.default_rng(3)
    psi0 = _rand_state(n, 4)
    rx, rz, _ = _random_sum(n, n_rot, 5)
    th = rng.uniform(-np.pi, np.pi, n_rot)
    hx, hz, co = _random_sum(n, 9, 6)
    e, grad = gradient_forward(psi0, rx, rz, th, hx, hz, co)
    assert abs(e - energy(psi0, rx, rz, th, hx, hz, co)) < 1e-14
    for j in range(n_rot):
        up, dn = th.copy(), th.copy()
        up[j] += h
        dn[j] -= h
        fd = (energy(psi0, rx, rz, up, hx, hz, co) - energy(psi0, rx, rz, dn, hx, hz, co)) / (2 * h)
        assert abs(grad[j] - fd) < 1e-8, (j, grad[j], fd)
    assert np.max(np.abs(grad)) > 1e-2


class HostChunk:
    """The chunk calls `hamiltonian` makes, on a numpy array of 2^k amplitudes (masks over PHYSICAL index bits)."""

    def __init__(self, psi):
        self.psi = np.array(psi, dtype=np.complex128)
        self.k = self.psi.size.bit_length() - 1
        self.calls = []

    def apply_pauli_rotations(self, x, z, th):
        self.calls.append(("rot", len(th)))
        self.psi = rotate_list(self.psi, x, z, th)
        return 1

    def apply_pauli_sum(self, src, x, z, coeffs):
        assert src is not self
        self.calls.append(("sum", len(coeffs)))
        self.psi = apply_sum(src.psi, x, z, coeffs)
        return 1

    def overlap_pauli(self, bra, x, z):
        self.calls.append(("ovl", len(x)))
        return matrix_elements(bra.psi, self.psi, x, z)

    def expectation(self, obs, l2p=None):
        obs = as_pauli_sum(obs, self.k if l2p is None else len(l2p))
        x, z = obs.masks(l2p)
        return obs.value(matrix_elements(self.psi, self.psi, x, z).real)

    def norm2(self):
        return float(np.vdot(self.psi, self.psi).real)


def _to_physical_state(logical, l2p):
    """The array a chunk holds when its logical qubit q lives on index bit l2p[q]."""
    i = np.arange(logical.size)
    y = np.zeros_like(i)
    for q, p in enumerate(l2p):
        y |= ((i >> p) & 1) << q
    return logical[y]


def _problem(n, n_rot, seed):
    rng = np.random.default_rng(seed)
    terms = [(float(rng.uniform(0.5, 1.5)), {q: p, q + 1: p}) for q in range(n - 1) for p in "XYZ"]
    terms += [(0.4, {}), (-0.6, {q: "X" for q in range(n)})]
    total = sum(abs(c) for c, _ in terms)
    obs = PauliSum([(c / total, ops) for c, ops in terms], n_qubits=n)
    rx, rz, _ = _random_sum(n, n_rot, seed + 1)
    return obs, (np.array(rx, dtype=np.uint64), np.array(rz, dtype=np.uint64), rng.uniform(-np.pi, np.pi, n_rot))


@pytest.mark.parametrize("permuted", [False, True], ids=["identity", "permuted"])
def test_adjoint_gradient_variance_and_apply_through_a_host_chunk(permuted):
    n, n_rot = 6, 10
    l2p = [int(p) for p in np.random.default_rng(8).permutation(n)] if permuted else None
    layout = list(range(n)) if l2p is None else l2p
    psi0 = _rand_state(n, 9)
    obs, rot = _problem(n, n_rot, 11)
    chunk, work = HostChunk(_to_physical_state(psi0, layout)), HostChunk(np.zeros(1 << n))
    start = chunk.psi.copy()
    e, grad = hamiltonian.adjoint_gradient(chunk, work, l2p, rot, obs)
    want_e, want = gradient_forward(psi0, *rot, obs.x, obs.z, obs.coeffs)
    assert abs(e - want_e) < 1e-13
    assert grad.shape == (n_rot,) and np.max(np.abs(grad - want)) < 1e-12, np.max(np.abs(grad - want))
    assert np.max(np.abs(grad)) > 1e-2
    assert np.max(np.abs(chunk.psi - start)) < 1e-14                      # psi_0 again
    # one forward call, H psi once, then per parameter one overlap and one inverse rotation on each chunk
    assert chunk.calls == [("rot", n_rot)] + [("ovl", 1), ("rot", 1)] * n_rot
    assert work.calls == [("sum", len(obs))] + [("rot", 1)] * n_rot

    hpsi = apply_sum(psi0, obs.x, obs.z, obs.coeffs)
    assert hamiltonian.apply(work, chunk, l2p, obs) == 1
    assert np.max(np.abs(work.psi - _to_physical_state(hpsi, layout))) < 1e-14
    mean = float(np.vdot(psi0, hpsi).real)
    assert abs(hamiltonian.variance(chunk, work, l2p, obs) - (float(np.vdot(hpsi, hpsi).real) - mean * mean)) < 1e-13
    got = hamiltonian.matrix_elements(chunk, work, l2p, obs)
    assert np.max(np.abs(got - matrix_elements(hpsi, psi0, obs.x, obs.z))) < 1e-13


def test_an_empty_rotation_list_and_list_forms():
    n = 4
    psi0 = _rand_state(n, 12)
    obs, _ = _problem(n, 1, 13)
    chunk, work = HostChunk(psi0), HostChunk(np.zeros(1 << n))
    e, grad = hamiltonian.adjoint_gradient(chunk, work, None, [], obs)
    assert grad.shape == (0,) and grad.dtype == np.float64
    assert abs(e - float(np.vdot(psi0, apply_sum(psi0, obs.x, obs.z, obs.coeffs)).real)) < 1e-14
    assert np.array_equal(chunk.psi, psi0)
    # (pauli, theta) pairs and (x, z, theta) triples; a repeated string is two parameters
    e, grad = hamiltonian.adjoint_gradient(chunk, work, None, [("X0 Z3", 0.2), ({1: "Y"}, -0.4), (0b1001, 0b1000, 0.2)], obs)
    want_e, want = gradient_forward(psi0, [1, 2, 9], [8, 2, 8], [0.2, -0.4, 0.2], obs.x, obs.z, obs.coeffs)
    assert abs(e - want_e) < 1e-13 and np.max(np.abs(grad - want)) < 1e-12


def test_argument_errors():
    n = 4
    obs, rot = _problem(n, 3, 14)
    chunk, work, small = HostChunk(_rand_state(n, 15)), HostChunk(np.zeros(1 << n)), HostChunk(np.zeros(1 << (n - 1)))
    before = chunk.psi.copy()
    with pytest.raises(ValueError):
        hamiltonian.adjoint_gradient(chunk, chunk, None, rot, obs)                   # the same chunk twice
    with pytest.raises(ValueError):
        hamiltonian.adjoint_gradient(chunk, small, None, rot, obs)                   # sizes differ
    with pytest.raises(ValueError):
        hamiltonian.adjoint_gradient(chunk, work, None, (rot[0], rot[1], rot[2][:2]), obs)
    with pytest.raises(ValueError):
        hamiltonian.adjoint_gradient(chunk, work, None, (rot[0], rot[1], np.array([0.1, np.nan, 0.2])), obs)
    with pytest.raises(ValueError):
        hamiltonian.adjoint_gradient(chunk, work, None, rot, PauliSum({"X5": 1.0}))   # an observable on more qubits
    with pytest.raises(ValueError):
        hamiltonian.adjoint_gradient(chunk, work, [0, 1, 2, 2], rot, obs)            # not a layout
    with pytest.raises(ValueError):
        hamiltonian.apply(chunk, chunk, None, obs)
    with pytest.raises(ValueError):
        hamiltonian.variance(chunk, small, None, obs)
    with pytest.raises(ValueError):
        hamiltonian.matrix_elements(chunk, small, None, obs)
    assert np.array_equal(chunk.psi, before) and not chunk.calls                     # refused before anything ran
