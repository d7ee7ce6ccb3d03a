"""Observables as weighted sums of Pauli strings, H = sum_t c_t P_t with real c_t (H is Hermitian).

Conventions (the same as `kernel/ref_dense.simulate`): qubit q is bit q of the logical amplitude index.  A Pauli string
is held as two masks over LOGICAL qubits, x = the qubits that carry X or Y and z = the qubits that carry Z or Y, so
with ny = popcount(x & z) (Y = i X Z):

    P|i> = i^ny (-1)^popcount(i & z) |i ^ x>,
    <psi|P|psi> = sum_i (-1)^popcount(i & z) Re(i^ny conj(psi_{i ^ x}) psi_i).

`masks(l2p)` moves the masks onto physical index bits (logical qubit q on bit l2p[q]); the device evaluates the
unnormalised <psi|P_t|psi> of every term (qsim_expectation_pauli) and `value` applies the coefficients on the host.

Accepted forms:
    PauliSum([(0.5, {0: "X", 3: "Z"}), (-1.0, {})], n_qubits=4)     # sparse: {qubit: letter}
    PauliSum({"X0 Z3": 0.5, "Y7": 2.0}, n_qubits=8)                  # sparse labels: letter + qubit, space separated
    PauliSum({"IXZ": 1.0})                                           # dense labels, qiskit order: the RIGHTMOST
                                                                     # character is qubit 0 (here X on 1, Z on 0)
Repeated strings are summed (in order of first appearance); "I" / "" / {} is the identity.
"""
from __future__ import annotations

import numbers
import re

import numpy as np

_LETTERS = {"I": (0, 0), "X": (1, 0), "Y": (1, 1), "Z": (0, 1)}
_SPARSE = re.compile(r"^([IXYZ])(\d+)$")


def _coeff(c) -> float:
    if isinstance(c, (bool, np.bool_)) or not isinstance(c, numbers.Number):
        raise ValueError(f"coefficient {c!r} is not a number")
    if isinstance(c, numbers.Complex) and not isinstance(c, numbers.Real):
        if complex(c).imag != 0:
            raise ValueError(f"complex coefficient {c!r}: a Pauli sum with complex weights is not Hermitian")
        c = complex(c).real
    c = float(c)
    if not np.isfinite(c):
        raise ValueError(f"coefficient {c!r} is not finite")
    return c


def _string_masks(ops: dict) -> tuple[int, int]:
    x = z = 0
    for q, letter in ops.items():
        if isinstance(q, (bool, np.bool_)) or not isinstance(q, numbers.Integral) or q < 0:
            raise ValueError(f"qubit {q!r} is not a non-negative integer")
        if not isinstance(letter, str) or letter.upper() not in _LETTERS:
            raise ValueError(f"bad Pauli letter {letter!r} on qubit {q} (X, Y, Z or I expected)")
        bx, bz = _LETTERS[letter.upper()]
        x |= bx << int(q)
        z |= bz << int(q)
    return x, z


def _parse_label(label: str) -> dict:
    """"X0 Z3 Y7" (sparse) or "IXZ" (dense, rightmost character = qubit 0) -> {qubit: letter}."""
    text = label.strip()
    if not text:
        return {}
    words = text.split()
    if all(_SPARSE.match(w.upper()) for w in words):
        ops: dict = {}
        for w in words:
            letter, q = _SPARSE.match(w.upper()).groups()
            q = int(q)
            if q in ops:
                raise ValueError(f"label {label!r}: qubit {q} appears twice")
            ops[q] = letter
        return ops
    if len(words) == 1:
        dense = words[0].upper()
        bad = [ch for ch in dense if ch not in _LETTERS]
        if bad:
            raise ValueError(f"label {label!r}: bad Pauli letter {bad[0]!r}")
        return {q: ch for q, ch in enumerate(reversed(dense))}
    raise ValueError(f"label {label!r}: expected 'X0 Z3 ...' or a dense string such as 'IXZ'")


class PauliSum:
    """sum_t coeffs[t] * P(x[t], z[t]) over logical qubits 0 .. n_qubits-1."""

    def __init__(self, terms, n_qubits: int | None = None):
        if isinstance(terms, dict):
            items = [(c, _parse_label(lab) if isinstance(lab, str) else lab) for lab, c in terms.items()]
            for lab, _ in terms.items():
                if not isinstance(lab, str):
                    raise ValueError(f"label {lab!r} is not a string")
        else:
            items = []
            for item in terms:
                if len(item) != 2:
                    raise ValueError(f"term {item!r}: expected (coeff, {{qubit: letter}})")
                c, ops = item
                items.append((c, _parse_label(ops) if isinstance(ops, str) else ops))
        acc: dict = {}
        top = -1
        for c, ops in items:
            if not isinstance(ops, dict):
                raise ValueError(f"Pauli string {ops!r}: expected {{qubit: letter}} or a label")
            x, z = _string_masks(ops)
            top = max(top, (x | z).bit_length() - 1)
            acc[(x, z)] = acc.get((x, z), 0.0) + _coeff(c)
        if n_qubits is None:
            n_qubits = top + 1
        if n_qubits < 0 or top >= n_qubits:
            raise ValueError(f"qubit {top} >= n_qubits = {n_qubits}")
        self.n_qubits = int(n_qubits)
        self.x = [k[0] for k in acc]
        self.z = [k[1] for k in acc]
        self.coeffs = np.array(list(acc.values()), dtype=np.float64)

    def __len__(self) -> int:
        return len(self.coeffs)

    def __repr__(self) -> str:
        return f"PauliSum({len(self)} terms on {self.n_qubits} qubits)"

    def labels(self) -> list[str]:
        """Sparse labels of the terms ("X0 Z3"; "I" for the identity)."""
        out = []
        for x, z in zip(self.x, self.z):
            words = []
            for q in range(max(x, z).bit_length()):
                bx, bz = (x >> q) & 1, (z >> q) & 1
                if bx or bz:
                    words.append(("Y" if bz else "X") + str(q) if bx else "Z" + str(q))
            out.append(" ".join(words) or "I")
        return out

    def masks(self, l2p=None) -> tuple[np.ndarray, np.ndarray]:
        """(x, z) as uint64 arrays over PHYSICAL index bits: logical qubit q lives on bit l2p[q] (None = identity)."""
        x = np.array(self.x, dtype=np.uint64)
        z = np.array(self.z, dtype=np.uint64)
        if l2p is None:
            return x, z
        l2p = [int(p) for p in l2p]
        if len(l2p) < self.n_qubits or len(set(l2p)) != len(l2p):
            raise ValueError(f"layout {l2p} does not place {self.n_qubits} qubits on distinct bits")
        px = np.zeros_like(x)
        pz = np.zeros_like(z)
        for q in range(self.n_qubits):
            px |= ((x >> np.uint64(q)) & np.uint64(1)) << np.uint64(l2p[q])
            pz |= ((z >> np.uint64(q)) & np.uint64(1)) << np.uint64(l2p[q])
        return px, pz

    def value(self, term_values) -> float:
        """sum_t coeffs[t] * term_values[t], in term order."""
        v = np.asarray(term_values, dtype=np.float64)
        if v.shape != self.coeffs.shape:
            raise ValueError(f"{v.size} term values for {len(self)} terms")
        total = 0.0
        for c, t in zip(self.coeffs, v):
            total += float(c) * float(t)
        return total


def as_pauli_sum(obs, n_qubits: int) -> PauliSum:
    """A PauliSum on n_qubits (a PauliSum, or anything its constructor accepts)."""
    if not isinstance(obs, PauliSum):
        obs = PauliSum(obs, n_qubits=n_qubits)
    if obs.n_qubits > n_qubits:
        raise ValueError(f"observable on {obs.n_qubits} qubits, state of {n_qubits}")
    return obs


def pauli_terms_np(psi: np.ndarray, x, z) -> np.ndarray:
    """numpy restatement: <psi|P_t|psi> = sum_i (-1)^popcount(i & z) Re(i^ny conj(psi_{i ^ x}) psi_i), unnormalised,
    for masks over the index bits of psi (the checker of the device kernels)."""
    psi = np.asarray(psi, dtype=np.complex128)
    i = np.arange(psi.size, dtype=np.uint64)
    out = []
    for xt, zt in zip(np.asarray(x, dtype=np.uint64), np.asarray(z, dtype=np.uint64)):
        ny = bin(int(xt) & int(zt)).count("1") & 3
        par = np.zeros(psi.size, dtype=np.uint64)
        v = i & zt
        while np.any(v):
            par ^= v & np.uint64(1)
            v >>= np.uint64(1)
        sign = 1.0 - 2.0 * par.astype(np.float64)
        c = (1j ** ny) * np.conj(psi[(i ^ xt).astype(np.int64)]) * psi
        out.append(float(np.sum(sign * c.real)))
    return np.array(out, dtype=np.float64)
