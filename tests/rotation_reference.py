"""Host reference of the Pauli rotation R = exp(-i theta P) = cos(theta) I - i sin(theta) P (NO factor 1/2 on theta):
P is applied as an operator by pauli_reference.apply_pauli (axis flips and sign vectors, no index arithmetic), so what
this shares with the device kernels is the definition alone.  One flip and one multiply per rotation: affordable at 2^22
amplitudes.  Pinned against scipy.linalg.expm of explicit Kronecker products and against the gate decomposition through
oracle.dense_oracle in tests/test_pauli_rotation_cpu.py.

Also here, for the tests that compare against the gate path: `rotation_gates`, the textbook decomposition of one rotation
into basis changes, a CNOT ladder and one RZ, as [(qubits, U)] with qubits[0] the MSB of a two-qubit matrix."""
import numpy as np

from tests.pauli_reference import apply_pauli


def rotate(psi: np.ndarray, x: int, z: int, theta: float) -> np.ndarray:
    """exp(-i theta P) |psi> for the string with X or Y on the bits of `x` and Z or Y on the bits of `z`."""
    psi = np.asarray(psi, dtype=np.complex128)
    return np.cos(theta) * psi - 1j * np.sin(theta) * apply_pauli(psi, int(x), int(z))


def rotate_list(psi: np.ndarray, xs, zs, thetas) -> np.ndarray:
    """The rotations applied first entry first."""
    for x, z, th in zip(xs, zs, thetas):
        psi = rotate(psi, int(x), int(z), float(th))
    return psi


LONG_N = 13
LONG_TILE = 0b1111110110111             # 11 tile bits, the line bits among them; bits 3 and 6 stay outside: four tiles


def long_rotation_list(count: int = 1030, seed: int = 60):
    """(x, z, thetas) of `count` rotations on LONG_N qubits that fit ONE tile: about a third Z-only strings, the others
    with X/Y on one to three bits of LONG_TILE; Z anywhere, the outer bits 3 and 6 included.  More than the 1024 rotations
    of a pass: the planner splits the list.  Shared by the device test and the check of this reference's own rounding."""
    rng = np.random.default_rng(seed)
    inside = [b for b in range(LONG_N) if (LONG_TILE >> b) & 1]
    x = [0 if rng.random() < 1 / 3 else int(sum(1 << int(b) for b in rng.choice(inside, size=int(rng.integers(1, 4)), replace=False)))
         for _ in range(count)]
    z = rng.integers(0, 1 << LONG_N, count)
    return np.array(x, dtype=np.uint64), z.astype(np.uint64), rng.uniform(-np.pi, np.pi, count)


_H = np.array([[1, 1], [1, -1]], dtype=np.complex128) / np.sqrt(2.0)
_SDG = np.diag([1.0, -1j]).astype(np.complex128)
_CNOT = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1], [0, 0, 1, 0]], dtype=np.complex128)    # control = MSB


def rotation_gates(x: int, z: int, theta: float) -> list:
    """exp(-i theta P) as gates, first gate first: per qubit the basis change B with B P_q B^+ = Z (X: H; Y: H S^+), a
    CNOT ladder that gathers the parity of the string's qubits on the highest one, RZ = diag(e^-i theta, e^+i theta)
    there, and everything undone.  The identity string is one global-phase matrix on qubit 0."""
    x, z = int(x), int(z)
    qs = [q for q in range((x | z).bit_length()) if ((x | z) >> q) & 1]
    if not qs:
        return [([0], np.exp(-1j * theta) * np.eye(2, dtype=np.complex128))]
    basis = []
    for q in qs:
        if (x >> q) & 1:
            basis.append(([q], _H @ _SDG if (z >> q) & 1 else _H))
    ladder = [([a, b], _CNOT) for a, b in zip(qs[:-1], qs[1:])]
    rz = ([qs[-1]], np.diag([np.exp(-1j * theta), np.exp(1j * theta)]))
    undo = [(q, U.conj().T) for q, U in reversed(basis)]
    return basis + ladder + [rz] + ladder[::-1] + undo
