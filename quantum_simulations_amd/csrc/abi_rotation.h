// abi_rotation.h -- C ABI: Pauli rotations exp(-i theta P) applied to a chunk in place (rot_kernels.h).
// Part of the single translation unit qsim_hip.hip (included there, in order; not a standalone header).
// R = cos(theta) I - i sin(theta) P: no factor 1/2 on theta.

extern "C" {
int qsim_plan_pauli_rotations(int n_local_qubits, int n, const uint64_t* x_masks, int32_t* pass_of, uint64_t* tile_masks, int* n_passes) {
  return plan_pauli_out(true, n_local_qubits, n, x_masks, pass_of, tile_masks, n_passes);
}

// The pass plan and the term table on the host (pauli_passes: in list order, the passes are runs of it), the table in
// the chunk's workspace, then per pass k_rot_tile or k_rot_wide on the chunk's stream; the kernels are not waited for.
// The table is copied from a vector of this call: hipMemcpyAsync from host memory that is not pinned copies before it
// returns (as documented, and as apply_dense_block relies on for the caller's matrix), so the vector may go with the
// call.
int qsim_apply_pauli_rotations(qsim_chunk* c, int n, const uint64_t* x_masks, const uint64_t* z_masks, const double* thetas, int* n_passes) {
  int rc = check_pauli_call(c, c, n, x_masks, z_masks, thetas, "theta", thetas, n_passes, "rotation", "qsim_apply_pauli_rotations");
  if (rc) return rc;
  PauliPasses pp;
  if ((rc = pauli_passes(kPauliRotation, c->k, n, x_masks, z_masks, thetas, &pp))) return rc;
  *n_passes = 0;
  if (n == 0) return QSIM_OK;
  if ((rc = ensure_work(c, pp.table.size()))) return rc;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemcpyAsync(c->work, pp.table.data(), pp.table.size(), hipMemcpyHostToDevice, c->stream));
  const bool nt = c->span_bytes > tuning().mall_bytes;
  const double bytes = 32.0 * (double)amps(c);
  const int np = (int)pp.plan.tile.size();
  for (int q = 0; q < np; ++q) {
    const int first = pp.first[(size_t)q];
    {
      ProfileScope prof(kClsRot, bytes, c->stream, nt);
      if (pp.wide_term[(size_t)q] >= 0) {
        const PauliTerm e = pp.entry(first);
        const int t = pp.wide_term[(size_t)q];
        RotWideArgs w;
        std::memset(&w, 0, sizeof w);
        w.amp = c->amp;
        w.half = amps(c) >> 1;
        w.x = x_masks[t];
        w.z = z_masks[t];
        w.h = 63 - __builtin_clzll(w.x);
        w.c = e.f0;
        w.fr = e.f1;
        w.fi = e.f2;
        QSIM_WITH_NT(hipLaunchKernelGGL((k_rot_wide<NT>), dim3(pauli_wide_grid(w.half)), dim3(kBlock), 0, c->stream, w));
      } else {
        RotArgs a;
        std::memset(&a, 0, sizeof a);
        a.amp = c->amp;
        a.terms = pp.at(c->work, first);
        a.w = tile_walk(c->k, pp.plan.tile[(size_t)q]);
        a.n_terms = pp.plan.count[(size_t)q];
        const unsigned grid = (unsigned)std::min<u64>(a.w.n_tiles, kExpMaxWg);
        QSIM_WITH_NT(hipLaunchKernelGGL((k_rot_tile<NT>), dim3(grid), dim3(kBlock), 0, c->stream, a));
      }
    }
    HIP_TRY(hipGetLastError());
  }
  *n_passes = np;
  return QSIM_OK;
}
}  // extern "C"
