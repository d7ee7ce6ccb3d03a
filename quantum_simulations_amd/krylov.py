"""Krylov-subspace solvers for a Pauli sum H = sum_t c_t P_t on device states: the Lanczos recurrence, a restarted
ground-state solver and Krylov time evolution in real and imaginary time, without ever downloading 2^n amplitudes.

    lanczos(chunk, work, l2p, obs, m)                   -> (alphas, betas, k);  chunk, work[0..k) := v_0 .. v_k
    ground_state(chunk, work, l2p, obs, m, tol, ...)    -> (energy, residual, restarts, h_applications);  chunk := psi_0
    evolve(chunk, work, l2p, obs, t, m, steps)          -> error estimate;  chunk := exp(-i t H) chunk

Everything here is host bookkeeping on small arrays, as in `hamiltonian`: the chunks' logical qubit q lives on index bit
l2p[q] (None: identity) and the layout goes into the masks; the amplitudes are touched by the device only, through three
chunk calls: H v out of place (`hamiltonian.apply_planned`: `apply_pauli_sum`, and with `fuse_diagonal` one diagonal pass
for the Z-only terms), `lincomb` (w := a w + sum a_s v_s with <v|w> and |w|^2 of the result
taken in the same pass) and `norm2`.  The caller supplies the work chunks: all of the state's size, on its
device, in its layout, and none of them the state itself.

Memory: a Krylov space of m steps keeps its basis, `chunk` plus m work chunks, m + 1 chunks in all.  A chunk of 30
qubits is 2^30 * 16 B = 16 GiB, so m = 16 needs 17 * 16 GiB = 272 GiB and m = 8 needs 9 * 16 GiB = 144 GiB; at 28
qubits (4 GiB each) m = 16 needs 68 GiB.
"""
from __future__ import annotations

import numpy as np

from quantum_simulations_amd import hamiltonian
from quantum_simulations_amd.evolution import n_qubits

GROUP = 4            # sources, and bras, of one `lincomb` call


def _check_chunks(chunk, work, m: int, least: int, what: str) -> None:
    m = int(m)
    if m < least:
        raise ValueError(f"{what}: m = {m}, at least {least}")
    if len(work) < m:
        raise ValueError(f"{what}: {len(work)} work chunks, m = {m} steps need {m} (m + 1 chunks with the state)")
    seen = [chunk]
    for w in work[:m]:
        if any(w is c for c in seen):
            raise ValueError(f"{what}: the state and the work chunks are all different chunks")
        if w.k != chunk.k:
            raise ValueError(f"{what}: chunks of {chunk.k} and {w.k} index bits")
        seen.append(w)


def _combine(dst, dst_coeff, vecs, coeffs, want_norm2: bool = False):
    """dst := dst_coeff dst + sum_i coeffs[i] vecs[i], in place, GROUP sources per pass (a_d = 1 for the later groups);
    the norm of the result is taken on the last pass."""
    if not len(vecs):
        return dst.lincomb(dst_coeff, want_norm2=want_norm2)[1]
    norm2 = None
    for g in range(0, len(vecs), GROUP):
        last = g + GROUP >= len(vecs)
        norm2 = dst.lincomb(dst_coeff if g == 0 else 1.0, vecs[g:g + GROUP], coeffs[g:g + GROUP], want_norm2=want_norm2 and last)[1]
    return norm2


def _normalise(chunk, what: str) -> float:
    """chunk := chunk / |chunk|; returns |chunk|."""
    n2 = chunk.norm2()
    if not np.isfinite(n2) or not n2 > 0.0:
        raise ValueError(f"{what}: the start vector has norm^2 = {n2!r}")
    norm = float(np.sqrt(n2))
    chunk.lincomb(1.0 / norm)
    return norm


def _apply_h(w, v, h) -> None:
    """w := H v, the one place where the solvers apply H (`h`: the plan of `_setup`)."""
    hamiltonian.apply_planned(w, v, h)


def _recurrence(basis, h, scale: float, m: int, reorth: bool, breakdown: float):
    """The Lanczos steps from the unit vector basis[0]: (alphas[k], betas[k], k) with betas[k - 1] the norm of the last
    residual.  basis[j + 1] := v_{j+1} for j < k (the last one only if the run did not break down)."""
    alphas, betas = [], []
    for j in range(m):
        v, w = basis[j], basis[j + 1]
        _apply_h(w, v, h)                                                         # w := H v_j, straight into its slot
        if j:
            dots, _ = w.lincomb(1.0, [basis[j - 1]], [-betas[j - 1]], bras=[v])   # w -= beta_{j-1} v_{j-1};  <v_j|w>
        else:
            dots, _ = w.lincomb(1.0, bras=[v])
        alpha = float(dots[0].real)
        _, n2 = w.lincomb(1.0, [v], [-alpha], want_norm2=True)                    # w -= alpha_j v_j;  |w|^2
        if reorth:                                                                # one classical Gram-Schmidt sweep
            kept = basis[:j + 1]
            over = np.concatenate([w.lincomb(1.0, bras=kept[g:g + GROUP])[0] for g in range(0, len(kept), GROUP)])
            n2 = _combine(w, 1.0, kept, -over, want_norm2=True)
        beta = float(np.sqrt(max(n2, 0.0)))
        alphas.append(alpha)
        betas.append(beta)
        if not beta > breakdown * scale:                                          # an invariant subspace: not an error
            break
        w.lincomb(1.0 / beta)
    return np.array(alphas), np.array(betas), len(alphas)


def _tridiagonal(alphas, betas, k: int):
    """(eigenvalues ascending, eigenvectors in columns) of the k x k Lanczos matrix."""
    T = np.diag(alphas[:k]) + np.diag(betas[:k - 1], 1) + np.diag(betas[:k - 1], -1)
    return np.linalg.eigh(T)


def _setup(chunk, l2p, obs, fuse_diagonal: bool):
    """(the plan of H for `_apply_h`, sum |c_t|)"""
    h = hamiltonian.plan(n_qubits(chunk, l2p), l2p, obs, fuse_diagonal)
    scale = float(np.sum(np.abs(h.coeffs))) + (float(np.sum(np.abs(h.diag_coeffs))) if h.diag_z is not None else 0.0)
    return h, scale


def lanczos(chunk, work, l2p, obs, m: int, reorth: bool = True, breakdown: float = 1e-12, fuse_diagonal: bool = False) -> tuple:
    """The Lanczos recurrence of a Pauli sum over LOGICAL qubits from v_0 = `chunk` (any norm but zero: it is normalised
    in place); `work` is a list of at least m chunks that become v_1 .. v_m.  Step j:
        w := H v_j, written straight into work[j];
        w -= beta_{j-1} v_{j-1} and alpha_j = Re <v_j|w> in one pass;  w -= alpha_j v_j and beta_j^2 = |w|^2 in one pass;
        with `reorth` one classical Gram-Schmidt sweep against v_0 .. v_j (read-only dots, 4 bras per pass, then the
        subtractions, 4 sources per pass, the norm taken on the last);
        v_{j+1} := w / beta_j.
    Returns (alphas, betas, k): the k x k tridiagonal matrix has alphas[0..k) on and betas[0..k-1) beside the diagonal,
    betas[k - 1] is the norm of the last residual.  k = m, or k = j + 1 when beta_j <= breakdown * sum |c_t|: the
    vectors span an invariant subspace (work[j] is then left unnormalised).  `fuse_diagonal`: every H application sends
    the Z-only terms through one diagonal pass (`hamiltonian.plan`)."""
    _check_chunks(chunk, work, m, 1, "lanczos")
    h, scale = _setup(chunk, l2p, obs, fuse_diagonal)
    _normalise(chunk, "lanczos")
    return _recurrence([chunk] + list(work[:int(m)]), h, scale, int(m), reorth, breakdown)


def ground_state(chunk, work, l2p, obs, m: int = 16, tol: float = 1e-8, max_restarts: int = 50, reorth: bool = True,
                 fuse_diagonal: bool = False) -> tuple:
    """The lowest eigenpair of a Pauli sum over LOGICAL qubits by restarted Lanczos, on the device.  On entry `chunk`
    holds the start vector (any norm but zero; it must overlap the ground state: a random state does); on return it holds
    the normalised eigenvector estimate psi.  One restart is: m Lanczos steps from psi, `numpy.linalg.eigh` of the
    tridiagonal matrix, the lowest Ritz vector sum_i y_i v_i built IN PLACE into `chunk` (= v_0) 4 sources per pass and
    normalised, and the TRUE residual: w := H psi into a free work chunk, E = Re <psi|w>, |w - E psi| in one more pass.
    The loop stops when that residual is <= tol or after `max_restarts` restarts (the caller compares `residual`).

    Needs m + 1 chunks in all: `chunk` plus m work chunks, 16 GiB each at 30 qubits (m = 16: 272 GiB; m = 8: 144 GiB).
    Returns (energy, residual, restarts, h_applications).  ValueError: fewer than m work chunks, m < 2, a zero start
    vector.  `fuse_diagonal`: as in `lanczos`."""
    _check_chunks(chunk, work, m, 2, "ground_state")
    m = int(m)
    h, scale = _setup(chunk, l2p, obs, fuse_diagonal)
    basis = [chunk] + list(work[:m])
    _normalise(chunk, "ground_state")
    energy = residual = float("nan")
    restarts = h_applications = 0
    while restarts < max(int(max_restarts), 1):
        alphas, betas, k = _recurrence(basis, h, scale, m, reorth, 1e-12)
        y = _tridiagonal(alphas, betas, k)[1][:, 0]
        n2 = _combine(chunk, y[0], basis[1:k], y[1:k], want_norm2=True)
        chunk.lincomb(1.0 / np.sqrt(n2))
        w = basis[1]
        _apply_h(w, chunk, h)
        energy = float(w.lincomb(1.0, bras=[chunk])[0][0].real)
        residual = float(np.sqrt(max(w.lincomb(1.0, [chunk], [-energy], want_norm2=True)[1], 0.0)))
        restarts += 1
        h_applications += k + 1
        if residual <= tol:
            break
    return energy, residual, restarts, h_applications


def evolve(chunk, work, l2p, obs, t, m: int = 16, steps: int = 1, fuse_diagonal: bool = False) -> float:
    """chunk := exp(-i t H) chunk for a Pauli sum over LOGICAL qubits, by `steps` Krylov steps of length dt = t / steps:
    m Lanczos steps from psi / |psi|, c = Y exp(-i dt Lambda) Y^T e_1 from the eigen-decomposition of the tridiagonal
    matrix on the host, and psi := |psi| sum_i c_i v_i built in place, 4 sources per pass.  `t` may be complex:
    t = -i tau is imaginary-time evolution exp(-tau H), whose result is NOT normalised (like every readout here).
    Returns the sum over the steps of |psi| beta_k |c_k|, the usual a-posteriori estimate of the l2 error.
    Needs m work chunks (see `ground_state`).  ValueError: fewer than m work chunks, m < 1, steps < 1, a time that is
    not finite, a zero state.  `fuse_diagonal`: as in `lanczos`."""
    _check_chunks(chunk, work, m, 1, "evolve")
    m, steps, t = int(m), int(steps), complex(t)
    if steps < 1:
        raise ValueError(f"evolve: steps = {steps}, at least one")
    if not np.isfinite(t):
        raise ValueError(f"evolve: time {t!r} is not finite")
    h, scale = _setup(chunk, l2p, obs, fuse_diagonal)
    basis = [chunk] + list(work[:m])
    dt = t / steps
    estimate = 0.0
    for _ in range(steps):
        norm = _normalise(chunk, "evolve")
        alphas, betas, k = _recurrence(basis, h, scale, m, True, 1e-12)
        lam, Y = _tridiagonal(alphas, betas, k)
        c = norm * (Y @ (np.exp(-1j * dt * lam) * Y[0, :]))
        _combine(chunk, c[0], basis[1:k], c[1:k])
        estimate += float(betas[k - 1] * abs(c[k - 1]))
    return estimate
