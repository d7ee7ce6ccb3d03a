"""What the tests of the on-device checkers (tests/test_gpu_checkers.py) share: the launch widths of the kernels under
test, the indices at which a reduction can go blind, the closed-form states in double and in long double, and the numpy
restatement of the random fill.  No GPU in here."""
from __future__ import annotations

import numpy as np

from oracle import dense_oracle as orc
from tests.cpu_shard_backend import _fp_mix

# The documented values of the library's launch constants.  tests/test_checkers_cpu.py reads them back from the sources:
# if one changes, the sizes below no longer reach the grid-stride loops and the tests have to be revisited.
K_BLOCK = 256             # kBlock (csrc/gate_kernels.h): threads of a workgroup
K_REDUCE_BLOCKS = 2048    # kReduceBlocks (csrc/readout_kernels.h): workgroups of the closed form and the norm
STREAM_GRID_MAX = 8192    # the cap of stream_grid (csrc/state_kernels.h): workgroups of the whole-state kernels

T_REDUCE = K_REDUCE_BLOCKS * K_BLOCK              # 2^19 threads: qsim_max_abs_err_closed_form(_perm), qsim_norm2
T_FINGERPRINT = (K_REDUCE_BLOCKS // 2) * K_BLOCK  # 2^18 threads: qsim_fingerprint launches kReduceBlocks / 2 workgroups
T_STREAM = STREAM_GRID_MAX * K_BLOCK              # 2^21 threads: fill, random fill, scale, count and append


def edge_indices(k: int, threads: int, seed: int = 0) -> list[int]:
    """The indices of a chunk of k qubits where a kernel of `threads` threads can go wrong: the ends of a wave and of a
    workgroup, both sides of the first stride and the end of the second, the last index, and eight seeded random ones."""
    size = 1 << k
    fixed = [0, 63, 64, 255, 256, threads - 1, threads, threads + 255, 2 * threads - 1, size - 1]
    rand = np.random.default_rng(1000 * k + seed).integers(0, size, size=8)
    return sorted({int(i) for i in fixed + list(rand) if 0 <= i < size})


def logical_index(x: np.ndarray, log_to_phys=None) -> np.ndarray:
    """y(x): bit q of y = bit log_to_phys[q] of x (None: identity)."""
    x = np.asarray(x, dtype=np.int64)
    if log_to_phys is None:
        return x
    y = np.zeros_like(x)
    for q, p in enumerate(log_to_phys):
        y |= ((x >> p) & 1) << q
    return y


def closed_form(kind: str, n_total: int, y: np.ndarray) -> np.ndarray:
    """complex128 amplitudes of the GHZ / GHZ+QFT state of n_total qubits at the logical indices y (the closed forms of
    oracle/dense_oracle.py)."""
    y = np.asarray(y, dtype=np.int64)
    if kind == "ghz":
        return np.where((y == 0) | (y == (1 << n_total) - 1), 2.0 ** -0.5, 0.0).astype(np.complex128)
    if kind == "ghz_qft":
        return orc.ghz_qft_closed_form(n_total, y)
    raise ValueError(kind)


def closed_form_longdouble(kind: str, n_total: int, y: np.ndarray):
    """(re, im) of the same amplitudes evaluated in long double (y / 2^n is exact there)."""
    y = np.asarray(y, dtype=np.int64)
    ld = np.longdouble
    if kind == "ghz":
        re = np.where((y == 0) | (y == (1 << n_total) - 1), np.sqrt(ld(0.5)), ld(0))
        return re, np.zeros(y.shape, dtype=ld)
    pi = ld(4) * np.arctan(ld(1))
    ang = -ld(2) * pi * (y.astype(ld) / ld(2) ** n_total)
    amp = ld(2) ** (-(ld(n_total) + ld(1)) / ld(2))
    return amp * (ld(1) + np.cos(ang)), amp * np.sin(ang)


def host_state_error(kind: str, n_total: int, y: np.ndarray, psi: np.ndarray) -> float:
    """max |psi - long double closed form|: what the double-precision host state itself is off by."""
    re, im = closed_form_longdouble(kind, n_total, y)
    return float(np.max(np.hypot(psi.real.astype(np.longdouble) - re, psi.imag.astype(np.longdouble) - im)))


def random_fill_uniforms(seed: int, first: int, count: int) -> np.ndarray:
    """u(j) = (fp_mix(seed + j) >> 11) * 2^-52 - 1 for j = first .. first + count - 1 (k_fill_random, csrc/state_kernels.h)."""
    with np.errstate(over="ignore"):
        j = np.uint64(seed) + np.arange(first, first + count, dtype=np.uint64)
    return (_fp_mix(j) >> np.uint64(11)).astype(np.float64) * 2.0 ** -52 - 1.0


def random_fill_norm2(seed: int, k: int) -> np.longdouble:
    """sum of u(j)^2 over the 2^(k+1) uniforms of a chunk of k qubits, in long double."""
    u = random_fill_uniforms(seed, 0, 2 << k).astype(np.longdouble)
    return np.sum(u * u)


def random_fill_amplitudes(seed: int, k: int, first: int = 0, count: int | None = None, norm2=None) -> np.ndarray:
    """Amplitudes first .. first + count - 1 of qsim_init_random(seed) on a chunk of k qubits: (u(2i), u(2i + 1)) divided
    by the square root of the long double norm."""
    count = (1 << k) - first if count is None else count
    norm2 = random_fill_norm2(seed, k) if norm2 is None else norm2
    u = random_fill_uniforms(seed, 2 * first, 2 * count).astype(np.longdouble) / np.sqrt(norm2)
    return u.astype(np.float64).view(np.complex128)


def bit_equal(a: np.ndarray, b: np.ndarray) -> bool:
    """Same bits (a -0.0 is not a 0.0, a NaN equals itself)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
