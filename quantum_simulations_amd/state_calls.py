"""The calls on "a state in a layout", once: `StateCalls` is inherited by `runner.engine.SingleGpuEngine` and by
`runner.single_node.HbmStateBuffer` (whose module functions forward here), so a new feature adds its call in one place.

A holder has `self.state` (the chunk of the whole state) and `self.l2p` (logical qubit q on index bit l2p[q]; None:
identity).  Every call runs on the device through that layout -- it goes into the masks and qubit lists, the state does
not move, nothing is downloaded or permuted.  Two hooks are all that differs between the holders:
    _second_chunk()    a context manager that yields the ONE scratch chunk of `variance`, `gradient`, `qaoa_gradient` and
                       the default `out` of `apply_observable`: allocated for the call and closed on every exit path (the
                       buffer), unless the holder keeps one (the engine: allocated on first use, closed with it);
    _state_written()   called by every call that writes the state, BEFORE it does (the engine forgets that the state is
                       |0..0>; a call that then fails has cost at most a SWAP pass later, never a relabelled state).
The m chunks of the Krylov calls are neither: `_fresh_chunks` allocates them for the call and closes them, for both."""
from __future__ import annotations

from contextlib import contextmanager, nullcontext

import numpy as np

from quantum_simulations_amd import diagonal, evolution, hamiltonian, krylov, readout
from quantum_simulations_amd.kernel.device import DeviceChunk
from quantum_simulations_amd.observable import as_pauli_sum


class StateCalls:
    def _state_written(self) -> None:
        pass

    def _new_chunk(self):
        return DeviceChunk.empty(self.state.k, self.state.device)

    @contextmanager
    def _fresh_chunks(self, count: int):
        """`count` chunks of the state's size for the `with` block; closed also when an allocation or the block raises."""
        work = []
        try:
            for _ in range(max(int(count), 0)):
                work.append(self._new_chunk())
            yield work
        finally:
            for c in work:
                c.close()

    @contextmanager
    def _second_chunk(self):
        """The default policy: a second chunk for one call, closed on every exit path (the engine keeps one instead)."""
        with self._fresh_chunks(1) as (work,):
            yield work

    # ---- readout: the state is only read -----------------------------------------------------------------------------
    def expectation(self, obs, per_term=False, fuse_diagonal=False):
        """<psi|H|psi> (unnormalised) of a Pauli sum over LOGICAL qubits (observable.PauliSum or what it accepts); with
        `per_term` the array of <psi|P_t|psi> in term order.  `fuse_diagonal`: the Z-only terms go through one
        Walsh-Hadamard pass (`readout.expectation`).  The per-term Z values and the ZZ correlators of the state are
        `diagonal.term_values` / `diagonal.correlations` on (`self.state`, `self.l2p`)."""
        return readout.expectation(self.state, self.l2p, obs, per_term, fuse_diagonal)

    def diagonal_moments(self, obs) -> tuple:
        """(<D>, <D^2> - <D>^2) of a diagonal Pauli sum over LOGICAL qubits in the NORMALISED state, one read-only pass."""
        return diagonal.moments(self.state, self.l2p, obs)

    def reduced_density_matrix(self, qubits) -> np.ndarray:
        """Reduced density matrix (unnormalised, complex128 (2^r, 2^r)) of 1 to 6 LOGICAL qubits, bit j of a row or
        column index = qubit qubits[j]."""
        return readout.reduced_density_matrix(self.state, self.l2p, qubits)

    def sample(self, shots: int, seed: int = 0, qubits=None) -> np.ndarray:
        """`shots` samples of the register (`sampling.draw(shots, seed)` gives the uniforms): LOGICAL basis-state indices
        as uint64, or with `qubits` the marginal values (bit j = qubit qubits[j]); `sampling.counts` counts them."""
        return readout.sample(self.state, self.l2p, shots, seed, qubits)

    def apply_observable(self, obs, out=None, fuse_diagonal: bool = False):
        """H|psi> for a Pauli sum over LOGICAL qubits, written into `out` (a chunk of the state's size on its device;
        default: the holder's second chunk, which `variance`, `gradient` and `qaoa_gradient` overwrite) IN THE STATE'S
        CURRENT LAYOUT `self.l2p`.  Returns that chunk; `out.last_pauli_sum_passes` = the HBM passes made by the per-term
        path.  `fuse_diagonal`: the Z-only terms go through one diagonal pass more (`hamiltonian.apply`)."""
        with (self._second_chunk() if out is None else nullcontext(out)) as out:
            hamiltonian.apply(out, self.state, self.l2p, obs, fuse_diagonal)
        return out

    def variance(self, obs, fuse_diagonal: bool = False) -> float:
        """<H^2> - <H>^2 (unnormalised: norm2(H psi) - <psi|H|psi>^2) of a Pauli sum over LOGICAL qubits; the second
        chunk is overwritten.  `fuse_diagonal`: as in `apply_observable`."""
        with self._second_chunk() as work:
            return hamiltonian.variance(self.state, work, self.l2p, obs, fuse_diagonal)

    def overlap_with(self, chunk, obs=None):
        """<chunk|psi> (obs None: a complex number), or <chunk|H|psi> = sum_t c_t <chunk|P_t|psi> for a Pauli sum over
        LOGICAL qubits; `chunk` holds a state of the same size in the state's current layout `self.l2p` (what
        `apply_observable` writes, or a copy of an earlier state).  Neither state moves."""
        if obs is None:
            return self.state.overlap(chunk)
        obs = as_pauli_sum(obs, self.state.k)
        terms = hamiltonian.matrix_elements(self.state, chunk, self.l2p, obs)
        return complex(sum(float(c) * complex(v) for c, v in zip(obs.coeffs, terms)))

    # ---- calls that write the state ------------------------------------------------------------------------------------
    def apply_pauli_rotations(self, rotations) -> int:
        """psi := exp(-i theta P) psi for every entry of `rotations`, first entry first.  No factor 1/2 on theta.
        `rotations`: the (x, z, theta) arrays of `evolution.trotter_rotations` over LOGICAL qubits, or a list of
        (pauli, theta) pairs / (x, z, theta) triples (`evolution.rotation`).  Returns the HBM passes made."""
        self._state_written()
        return evolution.apply_rotations(self.state, self.l2p, rotations)

    def evolve(self, obs, t, steps: int = 1, order: int = 1, fuse_diagonal: bool = False) -> int:
        """exp(-i t H) psi by a product formula (`evolution.trotter_rotations`: order 1 or the symmetric order 2,
        `steps` steps) of the Pauli sum H over LOGICAL qubits.  `fuse_diagonal`: runs of Z-only rotations go through one
        diagonal phase pass each (`evolution.apply_rotations`).  Returns the HBM passes made."""
        self._state_written()
        return evolution.evolve(self.state, self.l2p, obs, t, steps, order, fuse_diagonal)

    def apply_diagonal_phase(self, obs, gamma) -> int:
        """psi := exp(-i gamma D) psi for a diagonal Pauli sum D (Z and identity only) over LOGICAL qubits: ONE pass
        whatever the number of terms.  No factor 1/2 (`diagonal.apply_phase`).  Returns the HBM passes made."""
        self._state_written()
        return diagonal.apply_phase(self.state, self.l2p, obs, gamma)

    def qaoa(self, cost, gammas, betas) -> int:
        """QAOA layers on the current state: per layer exp(-i gamma_l C) for the diagonal cost C over LOGICAL qubits
        (one pass), then exp(-i beta_l X_q) on every qubit; no factor 1/2 (`diagonal.qaoa`).  Returns the HBM passes."""
        self._state_written()
        return diagonal.qaoa(self.state, self.l2p, cost, gammas, betas)

    def qaoa_gradient(self, cost, gammas, betas) -> tuple:
        """(E, dE/dgammas, dE/dbetas) of E = <psi|C|psi> with psi = the QAOA circuit of `qaoa` applied to the CURRENT
        state, by the adjoint method (`diagonal.qaoa_gradient`: per layer one overlap with the n mixer strings, one
        diagonal overlap pass and the two inverse layers on two chunks); no factor 1/2, unnormalised.  The state is the
        same afterwards up to rounding; the second chunk is overwritten."""
        self._state_written()
        with self._second_chunk() as work:
            return diagonal.qaoa_gradient(self.state, work, self.l2p, cost, gammas, betas)

    def gradient(self, rotations, obs) -> tuple:
        """(E, dE/dtheta) of E = <psi(theta)|H|psi(theta)> with psi(theta) = the rotation list (every entry its own
        parameter, exp(-i theta P) without a factor 1/2; forms as in `apply_pauli_rotations`) applied to the CURRENT
        state, by the adjoint method (`hamiltonian.adjoint_gradient`: one forward run, then one overlap and two
        single-rotation passes per parameter).  The state is the same afterwards up to rounding; overwrites the second chunk."""
        self._state_written()
        with self._second_chunk() as work:
            return hamiltonian.adjoint_gradient(self.state, work, self.l2p, rotations, obs)

    def ground_state(self, obs, m: int = 16, tol: float = 1e-8, max_restarts: int = 50, fuse_diagonal: bool = False) -> tuple:
        """The lowest eigenpair of a Pauli sum over LOGICAL qubits by restarted Lanczos (`krylov.ground_state`), started
        from the CURRENT state, which must overlap the ground state (a random state does) and is replaced by the
        normalised eigenvector estimate in the current layout.  m work chunks are allocated for the call and closed; the
        second chunk is not touched.  Returns (energy, residual |H psi - E psi|, restarts, H applications).
        `fuse_diagonal`: as in `apply_observable`, for every H application."""
        self._state_written()
        with self._fresh_chunks(m) as work:
            return krylov.ground_state(self.state, work, self.l2p, obs, m, tol, max_restarts, fuse_diagonal=fuse_diagonal)

    def evolve_krylov(self, obs, t, m: int = 16, steps: int = 1, fuse_diagonal: bool = False) -> float:
        """psi := exp(-i t H) psi to Krylov accuracy (`krylov.evolve`: `steps` steps of m Lanczos vectors each) for a
        Pauli sum over LOGICAL qubits; t = -i tau gives exp(-tau H) psi, unnormalised.  Work chunks as in `ground_state`.
        Returns the a-posteriori error estimate.  `fuse_diagonal`: as in `apply_observable`, for every H application."""
        self._state_written()
        with self._fresh_chunks(m) as work:
            return krylov.evolve(self.state, work, self.l2p, obs, t, m, steps, fuse_diagonal)
