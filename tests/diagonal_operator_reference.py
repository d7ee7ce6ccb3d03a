"""numpy reference of the diagonal Pauli sum D = sum_t c_t Z^{z_t} as an OPERATOR (qsim_apply_diagonal_sum,
qsim_overlap_diagonal) and of the QAOA gradient, on dense vectors; E(i) is tests/diagonal_reference.energies, the direct
sum over the terms.

    apply_sum(psi, z, c)                          -> D psi
    matrix_element(ket, bra, z, c)                -> (<bra|ket>, <bra|D|ket>), unnormalised
    qaoa_state / qaoa_energy(psi, z, c, g, b)     -> the circuit of `diagonal.qaoa` and <psi|C|psi> after it
    qaoa_gradient(psi, z, c, gammas, betas)       -> (E, dE/dgammas, dE/dbetas), each derivative state run FORWARD
    HostChunk                                     -> FakeChunk with the two-chunk calls, recording them

The gradient here is not the adjoint sweep of `diagonal.qaoa_gradient`: for every parameter the derivative of the circuit,
(-i G) inserted after its layer, is propagated forward through the remaining layers and contracted with C psi, p^2 layer
applications in all.  It is itself checked against central differences of `qaoa_energy` (tests/test_diagonal_operator_cpu).
"""
import numpy as np

from tests import diagonal_reference as ref
from tests.rotation_reference import rotate_list
from tests.twostate_reference import apply_sum as pauli_apply_sum
from tests.twostate_reference import matrix_elements as pauli_matrix_elements


def _n(psi) -> int:
    return np.asarray(psi).size.bit_length() - 1


def apply_sum(psi, z, c) -> np.ndarray:
    psi = np.asarray(psi, dtype=np.complex128)
    return ref.energies(_n(psi), z, c) * psi


def matrix_element(ket, bra, z, c) -> tuple:
    ket, bra = np.asarray(ket, dtype=np.complex128), np.asarray(bra, dtype=np.complex128)
    return complex(np.vdot(bra, ket)), complex(np.vdot(bra, ref.energies(_n(ket), z, c) * ket))


def _mixer(psi, beta: float) -> np.ndarray:
    """exp(-i beta X_q) on every qubit."""
    n = _n(psi)
    return rotate_list(psi, [1 << q for q in range(n)], [0] * n, [float(beta)] * n)


def _mixer_sum(psi) -> np.ndarray:
    """B psi, B = sum_q X_q."""
    i = np.arange(psi.size)
    return sum(psi[i ^ (1 << q)] for q in range(_n(psi)))


def _layer(psi, z, c, gamma, beta) -> np.ndarray:
    return _mixer(ref.phase(psi, z, c, gamma), beta)


def qaoa_state(psi, z, c, gammas, betas) -> np.ndarray:
    psi = np.asarray(psi, dtype=np.complex128)
    for g, b in zip(gammas, betas):
        psi = _layer(psi, z, c, g, b)
    return psi


def qaoa_energy(psi, z, c, gammas, betas) -> float:
    out = qaoa_state(psi, z, c, gammas, betas)
    return float(np.vdot(out, apply_sum(out, z, c)).real)


def qaoa_gradient(psi, z, c, gammas, betas) -> tuple:
    """(E, dE/dgammas, dE/dbetas), unnormalised, no factor 1/2: dE/dtheta = 2 Re <C psi_final| d psi_final / d theta>."""
    gammas, betas = np.asarray(gammas, dtype=np.float64), np.asarray(betas, dtype=np.float64)
    p = gammas.size
    final = qaoa_state(psi, z, c, gammas, betas)
    lam = apply_sum(final, z, c)
    dg, db = np.zeros(p), np.zeros(p)
    cur = np.asarray(psi, dtype=np.complex128)
    for l in range(p):
        after_cost = ref.phase(cur, z, c, gammas[l])
        d_gamma = _mixer(-1j * apply_sum(after_cost, z, c), betas[l])      # d/dgamma of layer l: -i C after the phase
        cur = _mixer(after_cost, betas[l])
        d_beta = -1j * _mixer_sum(cur)                                     # d/dbeta: -i B after the mixer
        for m in range(l + 1, p):
            d_gamma = _layer(d_gamma, z, c, gammas[m], betas[m])
            d_beta = _layer(d_beta, z, c, gammas[m], betas[m])
        dg[l] = 2.0 * float(np.vdot(lam, d_gamma).real)
        db[l] = 2.0 * float(np.vdot(lam, d_beta).real)
    return float(np.vdot(final, lam).real), dg, db


class HostChunk(ref.FakeChunk):
    """FakeChunk with the calls `diagonal.qaoa_gradient`, `hamiltonian.apply(fuse_diagonal=True)` and `krylov` make on
    two chunks, masks over PHYSICAL index bits, every call recorded in `calls`."""

    def apply_diagonal_sum(self, src, z_masks, coeffs, accumulate=False):
        z, co = np.array(z_masks, dtype=np.uint64), np.array(coeffs, dtype=np.float64)
        assert src is not self or not accumulate
        self.calls.append(("diagonal_sum", z, co, bool(accumulate)))
        self.psi = (self.psi if accumulate else 0.0) + apply_sum(src.psi, z, co)

    def overlap_diagonal(self, bra, z_masks, coeffs):
        z, co = np.array(z_masks, dtype=np.uint64), np.array(coeffs, dtype=np.float64)
        self.calls.append(("diagonal_overlap", z, co))
        return matrix_element(self.psi, bra.psi, z, co)

    def apply_pauli_sum(self, src, x_masks, z_masks, coeffs):
        assert src is not self
        x, z, co = np.array(x_masks, dtype=np.uint64), np.array(z_masks, dtype=np.uint64), np.array(coeffs, dtype=np.float64)
        self.calls.append(("sum", x, z, co))
        self.psi = pauli_apply_sum(src.psi, x, z, co) if co.size else np.zeros_like(self.psi)
        return 1 if co.size else 0

    def overlap_pauli(self, bra, x_masks, z_masks):
        x, z = np.array(x_masks, dtype=np.uint64), np.array(z_masks, dtype=np.uint64)
        self.calls.append(("overlap", x, z))
        return pauli_matrix_elements(bra.psi, self.psi, x, z)

    def expectation(self, obs, l2p=None):
        x, z = obs.masks(l2p)
        return float(np.vdot(self.psi, pauli_apply_sum(self.psi, x, z, obs.coeffs)).real)

    def lincomb(self, dst_coeff, srcs=(), coeffs=(), bras=(), want_norm2=False):
        from tests.krylov_reference import lincomb
        srcs, bras = list(srcs), list(bras)
        self.psi, dots, norm2 = lincomb(self.psi, dst_coeff, [s.psi for s in srcs], coeffs, [b.psi for b in bras], want_norm2)
        return dots, norm2

    def norm2(self):
        return float(np.vdot(self.psi, self.psi).real)
