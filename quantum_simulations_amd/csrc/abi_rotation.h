// abi_rotation.h -- C ABI: Pauli rotations exp(-i theta P) applied to a chunk in place (rot_kernels.h).
// Part of the single translation unit qsim_hip.hip (included there, in order; not a standalone header).
// R = cos(theta) I - i sin(theta) P: no factor 1/2 on theta.

extern "C" {
int qsim_plan_pauli_rotations(int n_local_qubits, int n, const uint64_t* x_masks, int32_t* pass_of, uint64_t* tile_masks, int* n_passes) {
  if (!n_passes || (n > 0 && (!pass_of || !tile_masks)))
    return fail(QSIM_ERR_INVALID, "qsim_plan_pauli_rotations: null argument");
  RotPlan p;
  const int rc = plan_rotations(n_local_qubits, n, x_masks, &p);
  if (rc) return rc;
  for (int t = 0; t < n; ++t) pass_of[t] = p.pass_of[(size_t)t];
  for (size_t q = 0; q < p.tile.size(); ++q) tile_masks[q] = p.tile[q];
  *n_passes = (int)p.tile.size();
  return QSIM_OK;
}

// The pass plan on the host, one term table per call in the chunk's workspace (in list order: the passes are runs of
// it), then per pass k_rot_tile or k_rot_wide on the chunk's stream; the kernels are not waited for.  The table is
// copied from a vector of this call: hipMemcpyAsync from host memory that is not pinned copies before it returns (as
// documented, and as apply_dense_block relies on for the caller's matrix), so the vector may go with the call.
int qsim_apply_pauli_rotations(qsim_chunk* c, int n, const uint64_t* x_masks, const uint64_t* z_masks, const double* thetas, int* n_passes) {
  int rc = check_chunk(c, "qsim_apply_pauli_rotations");
  if (rc) return rc;
  if (n < 0) return fail(QSIM_ERR_INVALID, "qsim_apply_pauli_rotations: n = %d", n);
  if (!n_passes || (n > 0 && (!x_masks || !z_masks || !thetas)))
    return fail(QSIM_ERR_INVALID, "qsim_apply_pauli_rotations: null argument");
  if ((rc = require_no_parts(c, "qsim_apply_pauli_rotations"))) return rc;
  const int k = c->k;
  const u64 all = (1ull << k) - 1;
  for (int t = 0; t < n; ++t) {
    if ((x_masks[t] | z_masks[t]) & ~all)
      return fail(QSIM_ERR_NONLOCAL, "qsim_apply_pauli_rotations: rotation %d acts on index bit %d >= log2(chunk_size)=%d", t,
                  63 - __builtin_clzll((x_masks[t] | z_masks[t]) & ~all), k);
    if (!std::isfinite(thetas[t])) return fail(QSIM_ERR_INVALID, "qsim_apply_pauli_rotations: theta of rotation %d is not finite", t);
  }
  RotPlan p;
  if ((rc = plan_rotations(k, n, x_masks, &p))) return rc;
  *n_passes = 0;
  if (n == 0) return QSIM_OK;
  const int np = (int)p.tile.size();
  std::vector<RotTerm> table((size_t)n);
  std::memset(table.data(), 0, sizeof(RotTerm) * table.size());
  for (int t = 0; t < n; ++t) {
    const u64 T = p.tile[(size_t)p.pass_of[(size_t)t]];
    const u64 x = x_masks[t], z = z_masks[t];
    RotTerm& e = table[(size_t)t];
    rot_factors(x, z, thetas[t], &e.c, &e.fr, &e.fi);
    if (!T && x) continue;                          // wide: the masks go as launch arguments
    e.xi = (unsigned)exp_pext(x, T);
    e.zi = (unsigned)exp_pext(z & T, T);
    e.zo = z & ~T;
    e.h = e.xi ? 31 - __builtin_clz(e.xi) : -1;
  }
  if ((rc = ensure_work(c, sizeof(RotTerm) * (u64)n))) return rc;
  RotTerm* dev_table = static_cast<RotTerm*>(c->work);
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemcpyAsync(dev_table, table.data(), sizeof(RotTerm) * table.size(), hipMemcpyHostToDevice, c->stream));
  const bool nt = c->span_bytes > tuning().mall_bytes;
  const double bytes = 32.0 * (double)amps(c);
  for (int q = 0, first = 0; q < np; first += p.count[(size_t)q], ++q) {
    const u64 T = p.tile[(size_t)q];
    ProfileScope prof(12, bytes, c->stream, nt);
    if (!T && x_masks[first]) {
      const RotTerm& e = table[(size_t)first];
      RotWideArgs w;
      std::memset(&w, 0, sizeof w);
      w.amp = c->amp;
      w.half = amps(c) >> 1;
      w.x = x_masks[first];
      w.z = z_masks[first];
      w.h = 63 - __builtin_clzll(w.x);
      w.c = e.c;
      w.fr = e.fr;
      w.fi = e.fi;
      const unsigned grid = (unsigned)std::min<u64>(std::max<u64>(w.half / kBlock, 1), kExpMaxWg);
      QSIM_WITH_NT(hipLaunchKernelGGL((k_rot_wide<NT>), dim3(grid), dim3(kBlock), 0, c->stream, w));
    } else {
      RotArgs a;
      std::memset(&a, 0, sizeof a);
      a.amp = c->amp;
      a.terms = dev_table + first;
      a.tb = __builtin_popcountll(T);
      for (int b = 0, j = 0; b < k; ++b)
        if ((T >> b) & 1) a.tile_bit[j++] = b;
      a.outer_mask = all & ~T;
      a.n_tiles = 1ull << (k - a.tb);
      a.n_terms = p.count[(size_t)q];
      const unsigned grid = (unsigned)std::min<u64>(a.n_tiles, kExpMaxWg);
      QSIM_WITH_NT(hipLaunchKernelGGL((k_rot_tile<NT>), dim3(grid), dim3(kBlock), 0, c->stream, a));
    }
    HIP_TRY(hipGetLastError());
    prof.done(c->stream);
  }
  *n_passes = np;
  return QSIM_OK;
}
}  // extern "C"
