"""Closed forms on product states: the reference of the full-size tests (tests/test_gpu_fullsize_calls.py), where a host
copy of the state (8 to 64 GiB) is out of reach.  Plain numpy, numpy.longdouble where many terms are added.

A product state is an (n, 2) complex array f of normalised single-qubit states: qubit q is index bit q, so
psi_i = prod_q f[q, bit q of i].  A `ProductSum` is a list of (coeff, factors): sum_s coeff_s |f_s>.  Pauli strings
(masks (x, z) of physical bits, x: X or Y, z: Z or Y, Y = i X Z as in csrc/pauli_tile.h) map a product state to a product
state, so rotations exp(-i theta P) = cos(theta) I - i sin(theta) P (no factor 1/2), Pauli sums and diagonal phases of
few terms keep a state inside the ProductSums, and every number the device calls produce -- amplitudes, inner products,
expectation values, reduced density matrices, moments of a diagonal sum, the CDF of |amp|^2 -- costs O(n) per amplitude
or per pair of terms.  Every function is pinned against dense vectors and Kronecker matrices at n = 6 .. 10 in
tests/test_product_reference_cpu.py (bound 1e-13).
"""
import numpy as np

LD, CLD = np.longdouble, np.clongdouble
WINDOW = 4096


# ---- product states ------------------------------------------------------------------------------------------------------
def factors(n: int, seed: int, near: int = None, wobble: float = 0.2) -> np.ndarray:
    """(n, 2) normalised single-qubit states (cos(t/2), sin(t/2) e^{i p}): polar angle t in [0.3, pi - 0.3], phase p
    random, so no amplitude of the product vanishes.  `near`: a second seed -- the angles of `seed` perturbed by at
    most `wobble` each (t kept inside its interval), a state whose overlap with the first is O(1)."""
    rng = np.random.default_rng(seed)
    t = rng.uniform(0.3, np.pi - 0.3, n)
    p = rng.uniform(0.0, 2.0 * np.pi, n)
    if near is not None:
        rng = np.random.default_rng(near)
        t = np.clip(t + rng.uniform(-wobble, wobble, n), 0.3, np.pi - 0.3)
        p = p + rng.uniform(-wobble, wobble, n)
    return np.stack([np.cos(0.5 * t) + 0j, np.sin(0.5 * t) * np.exp(1j * p)], axis=1)


def state_ops(f: np.ndarray) -> list:
    """[(qubits, U)]: one unitary per qubit whose first column is the qubit's factor -- applied to |0..0> they build the
    product state on the device."""
    return [([q], np.array([[a, -np.conj(b)], [b, np.conj(a)]], dtype=np.complex128)) for q, (a, b) in enumerate(np.asarray(f))]


def _bits(indices, q: int) -> np.ndarray:
    return ((np.asarray(indices, dtype=np.uint64) >> np.uint64(q)) & np.uint64(1)).astype(np.intp)


def amplitudes(f: np.ndarray, indices) -> np.ndarray:
    """psi_i of the product state for every index of `indices` (the product over q, in long double)."""
    g = np.asarray(f).astype(CLD)
    out = np.ones(np.shape(indices), dtype=CLD)
    for q in range(g.shape[0]):
        out *= g[q][_bits(indices, q)]
    return out.astype(np.complex128)


def sum_amplitudes(ps, indices) -> np.ndarray:
    """The amplitudes of a ProductSum."""
    out = np.zeros(np.shape(indices), dtype=CLD)
    for c, f in ps:
        g = np.asarray(f).astype(CLD)
        term = np.full(np.shape(indices), CLD(c), dtype=CLD)
        for q in range(g.shape[0]):
            term *= g[q][_bits(indices, q)]
        out += term
    return out.astype(np.complex128)


# ---- Pauli strings on ProductSums ----------------------------------------------------------------------------------------
def pauli_on(f: np.ndarray, x: int, z: int) -> np.ndarray:
    """P |f>, factor by factor: X (a, b) = (b, a), Z (a, b) = (a, -b), Y (a, b) = i X Z (a, b) = (-i b, i a): the i^ny of
    csrc/pauli_tile.h sits on the factors that carry a Y."""
    x, z = int(x), int(z)
    out = np.array(f, dtype=np.complex128)
    if (x | z) >> out.shape[0]:
        raise ValueError(f"a mask has a bit >= {out.shape[0]}")
    for q in range(out.shape[0]):
        a, b = out[q]
        bx, bz = (x >> q) & 1, (z >> q) & 1
        if bx and bz:
            out[q] = (-1j * b, 1j * a)
        elif bx:
            out[q] = (b, a)
        elif bz:
            out[q] = (a, -b)
    return out


def commute(x1: int, z1: int, x2: int, z2: int) -> bool:
    return (bin(int(x1) & int(z2)).count("1") + bin(int(z1) & int(x2)).count("1")) % 2 == 0


def rotate(ps, x: int, z: int, theta: float) -> list:
    """exp(-i theta P) ps = cos(theta) ps - i sin(theta) P ps: twice the terms."""
    c, s = np.cos(float(theta)), np.sin(float(theta))
    return [(c * co, f) for co, f in ps] + [(-1j * s * co, pauli_on(f, x, z)) for co, f in ps]


def apply_sum(ps, xs, zs, coeffs) -> list:
    """sum_t coeffs[t] P_t ps."""
    return [(complex(c) * co, pauli_on(f, x, z)) for x, z, c in zip(xs, zs, coeffs) for co, f in ps]


def inner(a, b) -> complex:
    """<a|b> of two ProductSums: sum_st conj(a_s) b_t prod_q <fa_s[q]|fb_t[q]>, in long double."""
    total = CLD(0)
    fb = [(CLD(cb), np.asarray(g).astype(CLD)) for cb, g in b]
    for ca, f in a:
        fc = np.conj(np.asarray(f).astype(CLD))
        for cb, g in fb:
            total += np.conj(CLD(ca)) * cb * np.prod(np.sum(fc * g, axis=1))
    return complex(total)


def expectation(ps, x: int, z: int) -> float:
    """<ps|P|ps>, unnormalised."""
    return inner(ps, [(co, pauli_on(f, x, z)) for co, f in ps]).real


def rdm(ps, qubits) -> np.ndarray:
    """The reduced density matrix of `qubits`, unnormalised, as tests/rdm_reference.py defines it: rho[a][b] = sum over
    the other bits e of psi(e, a) conj(psi(e, b)), bit j of a (and of b) on index bit qubits[j]."""
    qs = [int(q) for q in qubits]
    r = len(qs)
    assert len(set(qs)) == r
    pat = np.arange(1 << r)
    rho = np.zeros((1 << r, 1 << r), dtype=CLD)
    terms = []
    for c, f in ps:
        g = np.asarray(f).astype(CLD)
        vec = np.full(1 << r, CLD(c), dtype=CLD)
        for j, q in enumerate(qs):
            vec *= g[q][(pat >> j) & 1]
        terms.append((g, vec))
    rest = [q for q in range(terms[0][0].shape[0]) if q not in qs]
    for gs, vs in terms:
        for gt, vt in terms:
            env = np.prod(np.sum(gs[rest] * np.conj(gt[rest]), axis=1)) if rest else CLD(1)
            rho += env * np.outer(vs, np.conj(vt))
    return rho.astype(np.complex128)


# ---- diagonal sums D = sum_t c_t Z^{z_t} ---------------------------------------------------------------------------------
def diag_energy(indices, z_masks, coeffs) -> np.ndarray:
    """E(i) = sum_t c_t (-1)^popcount(i & z_t) for every index of `indices`, the direct sum in long double."""
    i = np.asarray(indices, dtype=np.uint64).reshape(-1)
    z = np.asarray(z_masks, dtype=np.uint64).reshape(-1)
    c = np.asarray(coeffs, dtype=np.float64).reshape(-1).astype(LD)
    e = np.zeros(i.size, dtype=LD)
    for zt, ct in zip(z, c):
        par = np.bitwise_count(i & zt) & np.uint8(1)
        e += np.where(par == 1, -ct, ct)
    return e.reshape(np.shape(indices))


def diag_phase(indices, z_masks, coeffs, gamma: float) -> np.ndarray:
    """exp(-i gamma E(i)); the angle is reduced in long double before the double-precision exponential."""
    ang = LD(float(gamma)) * diag_energy(indices, z_masks, coeffs)
    two_pi = 2 * np.arctan2(LD(0), LD(-1))
    ang = ang - two_pi * np.round(ang / two_pi)
    return (np.cos(ang) - 1j * np.sin(ang)).astype(np.complex128)


def _z_products(f: np.ndarray, masks: np.ndarray) -> np.ndarray:
    """sum_i |psi_i|^2 (-1)^popcount(i & m) for every mask: prod over q of (|a|^2 - |b|^2) on the mask's bits and of
    (|a|^2 + |b|^2) on the others."""
    g = np.asarray(f).astype(CLD)
    p0, p1 = (g[:, 0] * np.conj(g[:, 0])).real, (g[:, 1] * np.conj(g[:, 1])).real
    out = np.ones(masks.shape, dtype=LD)
    for q in range(g.shape[0]):
        on = ((masks >> np.uint64(q)) & np.uint64(1)).astype(bool)
        out *= np.where(on, p0[q] - p1[q], p0[q] + p1[q])
    return out


def diag_moments(f: np.ndarray, z_masks, coeffs) -> tuple:
    """(sum p, sum p E, sum p E^2) with p = |psi|^2 of the product state: <D> = sum_t c_t prod_{q in z_t} <Z>_q and
    <D^2> = sum_tt' c_t c_t' prod over the bits of z_t ^ z_t' (Z^a Z^b = Z^(a ^ b))."""
    z = np.asarray(z_masks, dtype=np.uint64).reshape(-1)
    c = np.asarray(coeffs, dtype=np.float64).reshape(-1).astype(LD)
    norm = _z_products(f, np.zeros(1, dtype=np.uint64))[0]
    mean = np.sum(c * _z_products(f, z)) if z.size else LD(0)
    second = np.sum(np.outer(c, c) * _z_products(f, z[:, None] ^ z[None, :])) if z.size else LD(0)
    return float(norm), float(mean), float(second)


# ---- the CDF of |amp|^2 and the sampling criterion ------------------------------------------------------------------------
def cdf_interval(f: np.ndarray, i) -> tuple:
    """(sum_{j < i} p_j, p_i) in long double by the descent from the most significant bit: where bit q of i is set, every
    index that agrees with i above q and has bit q clear lies below i -- the weight of the bits above times |f[q, 0]|^2
    (times the whole weight of the bits below q)."""
    g = np.asarray(f).astype(CLD)
    n = g.shape[0]
    p = np.stack([(g[:, 0] * np.conj(g[:, 0])).real, (g[:, 1] * np.conj(g[:, 1])).real], axis=1)     # (n, 2) long double
    below_w = np.ones(n + 1, dtype=LD)                  # below_w[q] = prod_{q' < q} (p0 + p1)
    for q in range(n):
        below_w[q + 1] = below_w[q] * (p[q, 0] + p[q, 1])
    cum = np.zeros(np.shape(i), dtype=LD)
    w = np.ones(np.shape(i), dtype=LD)
    for q in reversed(range(n)):
        b = _bits(i, q)
        cum += np.where(b == 1, w * p[q, 0] * below_w[q], LD(0))
        w *= p[q][b]
    return cum, w


def shot_failures(f: np.ndarray, randnums, indices, rtol: float = 1e-12) -> np.ndarray:
    """The shots that miss the criterion of tests/test_gpu_sampling.py (empty: all right), with `cdf_interval` in place of
    the cumulative sum of a downloaded state: index i for uniform r is right iff
    P[i-1] - tol <= r * total <= P[i] + tol and p[i] > 0, tol = rtol * total."""
    i = np.asarray(indices, dtype=np.uint64)
    r = np.asarray(randnums, dtype=np.float64)
    assert i.shape == r.shape and not np.any(i >> np.uint64(np.asarray(f).shape[0]))
    below, p = cdf_interval(f, i)
    total = cdf_interval(f, np.array([(1 << np.asarray(f).shape[0]) - 1], dtype=np.uint64))
    total = total[0][0] + total[1][0]
    tol = LD(rtol) * total
    t = r.astype(LD) * total
    ok = (below - tol <= t) & (t <= below + p + tol) & (p > 0)
    return np.flatnonzero(~ok)


# ---- where the full-size tests look --------------------------------------------------------------------------------------
def windows(n: int) -> list:
    """[(offset, WINDOW)]: the start, the end, one seeded aligned offset in the upper half and, where the state reaches
    them, the windows that straddle the 4 GiB byte boundary (amplitude 2^28) and amplitude 2^31, and the ones that end
    at amplitudes 2^29 and 2^32."""
    size = 1 << n
    assert size >= 4 * WINDOW
    rng = np.random.default_rng(1000 + n)
    offs = [0]
    if size > (1 << 28):
        offs += [(1 << 28) - WINDOW // 2, (1 << 29) - WINDOW]
    offs.append(int(rng.integers(size // 2 // WINDOW, size // WINDOW - 1)) * WINDOW)
    if size > (1 << 31):
        offs.append((1 << 31) - WINDOW // 2)
    if size >= (1 << 32):
        offs.append((1 << 32) - WINDOW)
    offs.append(size - WINDOW)
    return [(o, WINDOW) for o in sorted(set(offs))]
