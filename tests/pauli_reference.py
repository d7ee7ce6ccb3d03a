"""A second host reference of <psi|P|psi>, independent of observable.pauli_terms_np: P is APPLIED to the state as an
operator on psi.reshape([2] * n) -- X flips the qubit's axis, Z multiplies it by [1, -1], Y = i X Z does both with the
factor i -- and the value is Re <psi|P psi>.  No index arithmetic and no parity loop: what it shares with the device
kernels and with pauli_terms_np is the definition alone.  One flip, one multiply and one dot product per term, so it
stays affordable at 2^22 amplitudes, where pauli_terms_np takes seconds per term.  Pinned against pauli_terms_np and
against explicit Kronecker products in tests/test_observable_cpu.py."""
import numpy as np


def apply_pauli(psi: np.ndarray, x: int, z: int) -> np.ndarray:
    """P |psi> for the string with X or Y on the bits of `x` and Z or Y on the bits of `z` (qubit q = bit q of the
    index = axis n - 1 - q of psi.reshape([2] * n))."""
    psi = np.asarray(psi, dtype=np.complex128)
    n = psi.size.bit_length() - 1
    if psi.ndim != 1 or psi.size != 1 << n or (int(x) | int(z)) >> n:
        raise ValueError("a state of 2^n amplitudes and masks over its n index bits expected")
    x, z = int(x), int(z)
    sign = np.ones(1)                                  # the Z factors of every axis, highest qubit first
    for q in reversed(range(n)):
        sign = np.multiply.outer(sign, np.array([1.0, -1.0]) if (z >> q) & 1 else np.ones(2))
    phi = psi.reshape([2] * n) * sign.reshape([2] * n)              # Z (and the Z of every Y = i X Z) acts first
    flip = [n - 1 - q for q in range(n) if (x >> q) & 1]
    if flip:
        phi = np.flip(phi, axis=flip)                  # X: (X phi)[b] = phi[b ^ 1] along the qubit's axis
    return (1j ** (bin(x & z).count("1") & 3)) * phi.reshape(-1)


def pauli_terms_operator(psi: np.ndarray, x_masks, z_masks) -> np.ndarray:
    """<psi|P_t|psi> (unnormalised) of every term: Re <psi|P_t psi> with P_t applied as above."""
    psi = np.asarray(psi, dtype=np.complex128)
    return np.array([np.vdot(psi, apply_pauli(psi, int(x), int(z))).real for x, z in zip(x_masks, z_masks)], dtype=np.float64)
