"""Pauli rotations and Trotter steps: lists of R = exp(-i theta P) for the device (qsim_apply_pauli_rotations).

Convention: NO factor 1/2.  exp(-i theta P) = cos(theta) I - i sin(theta) P, so the gate RZ(phi) is `rotation({q: "Z"},
phi / 2)` and one first-order Trotter step of H = sum_t c_t P_t over the time dt is the list exp(-i c_t dt P_t), t in
term order.  A Pauli string is two masks over LOGICAL qubits as in `observable`: x = the qubits that carry X or Y, z =
those that carry Z or Y.  Rotations do not commute: a list is applied first entry first.

    rotation(pauli, theta)                    -> (x, z, theta) of one rotation
    trotter_rotations(obs, t, steps, order)   -> (x, z, theta) arrays approximating exp(-i t H)
    to_physical(x, z, l2p)                    -> the masks on PHYSICAL index bits (logical qubit q on bit l2p[q])
    rotation_gates(x, z, theta)               -> the same rotation as 1- and 2-qubit gates (for engines without the native
                                                 call, and the baseline of tools/rotation_probe.py)

    diagonal_runs(x, min_run)                 -> how `fuse_diagonal` cuts a list: runs of Z-only rotations go through one
                                                 diagonal phase pass each (`diagonal`)

Everything here is host bookkeeping on small arrays; the amplitudes are touched by the device only
(`DeviceChunk.apply_pauli_rotations`, `SingleGpuEngine.evolve`, `single_node.evolve`).
"""
from __future__ import annotations

import numpy as np

from quantum_simulations_amd.observable import PauliSum, _parse_label, _string_masks, as_pauli_sum


def rotation(pauli, theta) -> tuple[int, int, float]:
    """(x, z, theta) of exp(-i theta P) -- no factor 1/2 -- for P given as {qubit: "X" | "Y" | "Z"} or as a label the
    way `observable.PauliSum` takes them ("X0 Z3", or dense "IXZ" with the rightmost character on qubit 0)."""
    ops = _parse_label(pauli) if isinstance(pauli, str) else pauli
    if not isinstance(ops, dict):
        raise ValueError(f"Pauli string {pauli!r}: expected {{qubit: letter}} or a label")
    theta = float(theta)
    if not np.isfinite(theta):
        raise ValueError(f"angle {theta!r} is not finite")
    x, z = _string_masks(ops)
    return x, z, theta


def as_rotation_arrays(rotations) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """A rotation list in the form the device call takes: the (x, z, theta) arrays of `trotter_rotations` as they are,
    or a sequence whose entries are (x, z, theta) triples or (pauli, theta) pairs (`rotation`'s arguments)."""
    if isinstance(rotations, tuple) and len(rotations) == 3 and all(isinstance(a, np.ndarray) for a in rotations):
        x, z, th = rotations
    else:
        triples = [r if len(r) == 3 else rotation(*r) for r in rotations]
        x, z, th = ([r[i] for r in triples] for i in range(3))
    x = np.asarray(x, dtype=np.uint64).reshape(-1)
    z = np.asarray(z, dtype=np.uint64).reshape(-1)
    th = np.asarray(th, dtype=np.float64).reshape(-1)
    if not x.shape == z.shape == th.shape:
        raise ValueError(f"rotation list: {x.size} x masks, {z.size} z masks, {th.size} angles")
    return x, z, th


def trotter_rotations(obs, t, steps: int = 1, order: int = 1) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(x, z, theta) over LOGICAL qubits of a product formula for exp(-i t H), H = sum_j c_j P_j a `PauliSum`, in the
    order the rotations are applied (theta without a factor 1/2: exp(-i theta P)).
      order 1: `steps` repetitions of every term in term order, theta_j = c_j t / steps   (error O(t^2 / steps));
      order 2: per step every term with half that angle in term order, then again in reverse order (the symmetric form,
               error O(t^3 / steps^2)).
    The identity term is kept, with x = z = 0: a global phase."""
    if not isinstance(obs, PauliSum):
        obs = PauliSum(obs)
    steps = int(steps)
    if steps < 1:
        raise ValueError(f"steps = {steps}: at least one")
    if order not in (1, 2):
        raise ValueError(f"order = {order!r}: 1 or 2")
    t = float(t)
    if not np.isfinite(t):
        raise ValueError(f"time {t!r} is not finite")
    x = np.array(obs.x, dtype=np.uint64)
    z = np.array(obs.z, dtype=np.uint64)
    th = obs.coeffs * (t / steps)
    if order == 2:
        x = np.concatenate([x, x[::-1]])
        z = np.concatenate([z, z[::-1]])
        th = np.concatenate([0.5 * th, 0.5 * th[::-1]])
    return np.tile(x, steps), np.tile(z, steps), np.tile(th, steps)


def n_qubits(chunk, l2p) -> int:
    """Logical qubits of a chunk in the layout l2p (None: identity); with `check_pair`, shared by the physics modules."""
    return chunk.k if l2p is None else len(l2p)


def check_pair(a, b, what: str) -> None:
    """The two chunks of a call: different objects of the same size."""
    if a is b:
        raise ValueError(f"{what}: two different chunks expected, got the same one twice")
    if a.k != b.k:
        raise ValueError(f"{what}: chunks of {a.k} and {b.k} index bits")


def to_physical(x, z, l2p) -> tuple[np.ndarray, np.ndarray]:
    """Masks over logical qubits -> masks over PHYSICAL index bits: logical qubit q lives on bit l2p[q] (None: identity)."""
    x = np.asarray(x, dtype=np.uint64).reshape(-1)
    z = np.asarray(z, dtype=np.uint64).reshape(-1)
    if l2p is None:
        return x.copy(), z.copy()
    l2p = [int(p) for p in l2p]
    top = max([int(m).bit_length() for m in x | z], default=0)
    if top > len(l2p) or len(set(l2p)) != len(l2p) or any(p < 0 or p > 63 for p in l2p):
        raise ValueError(f"layout {l2p} does not place {top} qubits on distinct bits")
    px, pz = np.zeros_like(x), np.zeros_like(z)
    for q, p in enumerate(l2p):
        px |= ((x >> np.uint64(q)) & np.uint64(1)) << np.uint64(p)
        pz |= ((z >> np.uint64(q)) & np.uint64(1)) << np.uint64(p)
    return px, pz


_H = np.array([[1, 1], [1, -1]], dtype=np.complex128) / np.sqrt(2.0)
_HSDG = _H @ np.diag([1.0, -1j])                     # Y -> Z: (H S^+) Y (H S^+)^+ = Z
_CNOT = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1], [0, 0, 1, 0]], dtype=np.complex128)    # control = first qubit


def rotation_gates(x: int, z: int, theta: float) -> list:
    """exp(-i theta P) decomposed into gates [(qubits, U)], first gate first: a basis change on every X (H) and Y (H S^+)
    qubit, a CNOT ladder that gathers the parity of the string on its highest qubit, diag(e^-i theta, e^+i theta) there
    (RZ(2 theta)), and the ladder and the basis changes undone: 2 (weight - 1) CNOTs and up to 2 weight + 1 one-qubit
    gates, where `DeviceChunk.apply_pauli_rotations` makes one butterfly.  The identity string becomes a global-phase
    matrix on qubit 0."""
    x, z, theta = int(x), int(z), float(theta)
    qs = [q for q in range((x | z).bit_length()) if ((x | z) >> q) & 1]
    if not qs:
        return [([0], np.exp(-1j * theta) * np.eye(2, dtype=np.complex128))]
    basis = [([q], _HSDG if (z >> q) & 1 else _H) for q in qs if (x >> q) & 1]
    ladder = [([a, b], _CNOT) for a, b in zip(qs[:-1], qs[1:])]
    rz = ([qs[-1]], np.diag([np.exp(-1j * theta), np.exp(1j * theta)]))
    return basis + ladder + [rz] + ladder[::-1] + [(q, U.conj().T) for q, U in reversed(basis)]


# fuse_diagonal: the shortest run of consecutive Z-only rotations that goes through ONE diagonal phase pass
# (`DeviceChunk.apply_diagonal_phase`) instead of the rotation pass.  On a list of its own the diagonal pass beats
# qsim_apply_pauli_rotations from ONE term on (by 1 % at one term, 10 % at 8, 45 x at 512), but inside a list a fused run
# is a pass of its own AND cuts the rotation pass around it in two: measured with a run in the middle of a rotation list,
# fusing loses up to 20 Z strings and wins from 24 on, at 28 and at 30 qubits (profiles/r22_diagonal_probe.json,
# "crossover": "same_list" and "run_inside_a_list").  The constant is the second figure.
DIAGONAL_MIN_RUN = 24


def diagonal_runs(x, min_run: int | None = None) -> list:
    """The rotation list cut for `fuse_diagonal`: [(first, end, diagonal)] in list order, `diagonal` true for every
    maximal run of at least `min_run` (None: DIAGONAL_MIN_RUN) consecutive rotations with x == 0; what lies between two
    such runs is one piece."""
    x = np.asarray(x, dtype=np.uint64).reshape(-1)
    min_run = DIAGONAL_MIN_RUN if min_run is None else min_run
    runs, t, n, start = [], 0, int(x.size), 0
    while t < n:
        if x[t] != 0:
            t += 1
            continue
        end = t
        while end < n and x[end] == 0:
            end += 1
        if end - t >= max(int(min_run), 1):
            if t > start:
                runs.append((start, t, False))
            runs.append((t, end, True))
            start = end
        t = end
    if n > start:
        runs.append((start, n, False))
    return runs


def apply_rotations(chunk, l2p, rotations, fuse_diagonal: bool = False) -> int:
    """The rotation list (over LOGICAL qubits, any form of `as_rotation_arrays`) applied to a chunk whose logical qubit q
    lives on index bit l2p[q] (None: identity); the state does not move.  `fuse_diagonal`: every maximal run of at least
    DIAGONAL_MIN_RUN consecutive Z-only rotations (they commute) is ONE diagonal phase pass (gamma = 1, c_t = theta_t:
    `DeviceChunk.apply_diagonal_phase`), the rest goes through the rotation call in order.  Returns the HBM passes made."""
    x, z, th = as_rotation_arrays(rotations)
    px, pz = to_physical(x, z, l2p)
    if not fuse_diagonal:
        return chunk.apply_pauli_rotations(px, pz, th)
    passes = 0
    for first, end, diagonal in diagonal_runs(px):
        if diagonal:
            chunk.apply_diagonal_phase(pz[first:end], th[first:end], 1.0)
            passes += 1
        else:
            passes += chunk.apply_pauli_rotations(px[first:end], pz[first:end], th[first:end])
    return passes


def evolve(chunk, l2p, obs, t, steps: int = 1, order: int = 1, fuse_diagonal: bool = False) -> int:
    """`trotter_rotations(obs, t, steps, order)` applied to the chunk through its layout (`fuse_diagonal`: as in
    `apply_rotations`).  Returns the HBM passes made."""
    return apply_rotations(chunk, l2p, trotter_rotations(as_pauli_sum(obs, n_qubits(chunk, l2p)), t, steps, order), fuse_diagonal)
