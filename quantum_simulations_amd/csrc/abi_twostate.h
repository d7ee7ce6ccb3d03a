// abi_twostate.h -- C ABI: what takes two chunks: a Pauli sum applied out of place (psum_kernels.h) and the matrix
// elements of Pauli strings between two states (ovl_kernels.h).
// Part of the single translation unit qsim_hip.hip (included there, in order; not a standalone header).
// The argument checks are check_pauli_call's and the cache policy is pair_streams' (abi_readout.h), with two chunks.

extern "C" {
// The plan of qsim_plan_expectation on the host, one term table per call in dst's workspace (terms in pass order), then
// per pass k_psum_tile or k_psum_wide on dst's stream: the first writes dst, the later ones accumulate.  The kernels
// are not waited for; the table is copied from a vector of this call (see qsim_apply_pauli_rotations).
int qsim_apply_pauli_sum(qsim_chunk* dst, const qsim_chunk* src, int n_terms, const uint64_t* x_masks, const uint64_t* z_masks,
                         const double* coeffs, int* n_passes) {
  const char* const what = "qsim_apply_pauli_sum";
  int rc = check_pauli_call(dst, src, n_terms, x_masks, z_masks, coeffs, "coefficient", coeffs, n_passes, "term", what);
  if (rc) return rc;
  if (dst->amp < src->amp + amps(src) && src->amp < dst->amp + amps(dst))
    return fail(QSIM_ERR_INVALID, "%s: dst and src overlap (the call is out of place)", what);
  const int k = dst->k;
  PauliPasses pp;
  if ((rc = pauli_passes(kPauliSum, k, n_terms, x_masks, z_masks, coeffs, &pp))) return rc;
  *n_passes = 0;
  HIP_TRY(hipSetDevice(dst->device));
  if (n_terms == 0) {
    hipLaunchKernelGGL(k_fill_zero, dim3(stream_grid(amps(dst))), dim3(kBlock), 0, dst->stream, dst->amp, amps(dst), 0);
    HIP_TRY(hipGetLastError());
    return QSIM_OK;
  }
  if ((rc = ensure_work(dst, pp.table.size()))) return rc;
  HIP_TRY(hipMemcpyAsync(dst->work, pp.table.data(), pp.table.size(), hipMemcpyHostToDevice, dst->stream));
  const bool nt = pair_streams(dst, src);
  const int np = (int)pp.plan.tile.size();
  for (int q = 0; q < np; ++q) {
    const bool acc = q > 0;
    const double bytes = (acc ? 48.0 : 32.0) * (double)amps(dst);
    {
      ProfileScope prof(kClsPsum, bytes, dst->stream, nt);
      if (pp.wide_term[(size_t)q] >= 0) {
        const int t = pp.wide_term[(size_t)q];
        PsumWideArgs w;
        std::memset(&w, 0, sizeof w);
        w.dst = dst->amp;
        w.src = src->amp;
        w.n = amps(dst);
        w.x = x_masks[t];
        w.z = z_masks[t];
        w.gr = pp.entry(pp.first[(size_t)q]).f0;
        w.gi = pp.entry(pp.first[(size_t)q]).f1;
        const unsigned grid = pauli_wide_grid(w.n);
        if (acc) QSIM_WITH_NT(hipLaunchKernelGGL((k_psum_wide<NT, true>), dim3(grid), dim3(kBlock), 0, dst->stream, w));
        else QSIM_WITH_NT(hipLaunchKernelGGL((k_psum_wide<NT, false>), dim3(grid), dim3(kBlock), 0, dst->stream, w));
      } else {
        PsumArgs a;
        std::memset(&a, 0, sizeof a);
        a.dst = dst->amp;
        a.src = src->amp;
        a.terms = pp.at(dst->work, pp.first[(size_t)q]);
        a.w = tile_walk(k, pp.plan.tile[(size_t)q]);
        a.n_terms = pp.plan.count[(size_t)q];
        const unsigned grid = (unsigned)std::min<u64>(a.w.n_tiles, kExpMaxWg);
        if (acc) QSIM_WITH_NT(hipLaunchKernelGGL((k_psum_tile<NT, true>), dim3(grid), dim3(kBlock), 0, dst->stream, a));
        else QSIM_WITH_NT(hipLaunchKernelGGL((k_psum_tile<NT, false>), dim3(grid), dim3(kBlock), 0, dst->stream, a));
      }
    }
    HIP_TRY(hipGetLastError());
  }
  *n_passes = np;
  return QSIM_OK;
}

// The same plan; per pass k_ovl_tile (or k_ovl_wide) and the rest of pauli_reduce_call, (re, im) per term, in the ket's
// workspace.  (A wide pass has up to kExpMaxWg rows of 2 doubles, a tile pass up to kOvlMaxWg rows of 2 * count.)
int qsim_overlap_pauli(qsim_chunk* ket, const qsim_chunk* bra, int n_terms, const uint64_t* x_masks, const uint64_t* z_masks,
                       double* out_re_im, int* n_passes) {
  int rc = check_pauli_call(ket, bra, n_terms, x_masks, z_masks, nullptr, nullptr, out_re_im, n_passes, "term", "qsim_overlap_pauli");
  if (rc) return rc;
  PauliPasses pp;
  if ((rc = pauli_passes(kPauliSum, ket->k, n_terms, x_masks, z_masks, nullptr, &pp))) return rc;
  *n_passes = 0;
  if (n_terms == 0) return QSIM_OK;
  const bool nt = pair_streams(ket, bra);
  const double bytes = 32.0 * (double)amps(ket);
  const auto launch = [&](int q, const PauliTerm* terms, double* partial, unsigned* rows) {
    {
      ProfileScope prof(kClsOvl, bytes, ket->stream, nt);
      if (pp.wide_term[(size_t)q] >= 0) {
        const int t = pp.wide_term[(size_t)q];
        OvlWideArgs w;
        std::memset(&w, 0, sizeof w);
        w.bra = bra->amp;
        w.ket = ket->amp;
        w.partial = partial;
        w.n = amps(ket);
        w.x = x_masks[t];
        w.z = z_masks[t];
        w.gr = pp.entry(pp.first[(size_t)q]).f0;
        w.gi = pp.entry(pp.first[(size_t)q]).f1;
        *rows = pauli_wide_grid(w.n);
        QSIM_WITH_NT(hipLaunchKernelGGL((k_ovl_wide<NT>), dim3(*rows), dim3(kBlock), 0, ket->stream, w));
      } else {
        OvlArgs a;
        std::memset(&a, 0, sizeof a);
        a.bra = bra->amp;
        a.ket = ket->amp;
        a.terms = terms;
        a.partial = partial;
        a.w = tile_walk(ket->k, pp.plan.tile[(size_t)q]);
        a.n_terms = pp.plan.count[(size_t)q];
        a.slices = pauli_slices(a.n_terms);
        *rows = (unsigned)std::min<u64>(a.w.n_tiles, kOvlMaxWg);
        QSIM_WITH_NT(hipLaunchKernelGGL((k_ovl_tile<NT>), dim3(*rows), dim3(kBlock), 0, ket->stream, a));
      }
    }
    HIP_TRY(hipGetLastError());
    return QSIM_OK;
  };
  return pauli_reduce_call(ket, pp, 2, kOvlMaxWg, launch, out_re_im, n_passes);
}
}  // extern "C"
