// abi_twostate.h -- C ABI: what takes two chunks: a Pauli sum applied out of place (psum_kernels.h) and the matrix
// elements of Pauli strings between two states (ovl_kernels.h).
// Part of the single translation unit qsim_hip.hip (included there, in order; not a standalone header).

// The checks both calls share, in this order: null arguments, n_terms, the pair (size, device, stream), pending parts,
// then term by term locality (and the coefficient, where there is one).
static int check_two_chunks(const qsim_chunk* a, const qsim_chunk* b, int n_terms, const uint64_t* x_masks, const uint64_t* z_masks,
                            const double* coeffs, bool want_coeffs, const void* out, const int* n_passes, const char* what) {
  int rc = check_chunk(a, what);
  if (rc || (rc = check_chunk(b, what))) return rc;
  if (n_terms < 0) return fail(QSIM_ERR_INVALID, "%s: n_terms = %d", what, n_terms);
  if (!n_passes || (n_terms > 0 && (!x_masks || !z_masks || !out || (want_coeffs && !coeffs))))
    return fail(QSIM_ERR_INVALID, "%s: null argument", what);
  if (a->k != b->k) return fail(QSIM_ERR_INVALID, "%s: chunks of %d and %d index bits", what, a->k, b->k);
  if (a->device != b->device) return fail(QSIM_ERR_INVALID, "%s: chunks live on different devices", what);
  if (a->stream != b->stream) return fail(QSIM_ERR_INVALID, "%s: chunks are bound to different streams", what);
  if ((rc = require_no_parts(a, what)) || (rc = require_no_parts(b, what))) return rc;
  const u64 all = (1ull << a->k) - 1;
  for (int t = 0; t < n_terms; ++t) {
    if ((x_masks[t] | z_masks[t]) & ~all)
      return fail(QSIM_ERR_NONLOCAL, "%s: term %d acts on index bit %d >= log2(chunk_size)=%d", what, t,
                  63 - __builtin_clzll((x_masks[t] | z_masks[t]) & ~all), a->k);
    if (want_coeffs && !std::isfinite(coeffs[t])) return fail(QSIM_ERR_INVALID, "%s: coefficient of term %d is not finite", what, t);
  }
  return QSIM_OK;
}

// Do the two chunks' allocations together exceed the Infinity Cache?  (Views of one parent share its allocation.)
static bool pair_streams(const qsim_chunk* a, const qsim_chunk* b) {
  u64 bytes = a->span_bytes;
  if (a->amp != b->amp && !(a->parent && a->parent == b->parent)) bytes += b->span_bytes;
  return bytes > tuning().mall_bytes;
}

extern "C" {
// The plan of qsim_plan_expectation on the host, one term table per call in dst's workspace (terms in pass order), then
// per pass k_psum_tile or k_psum_wide on dst's stream: the first writes dst, the later ones accumulate.  The kernels
// are not waited for; the table is copied from a vector of this call (see qsim_apply_pauli_rotations).
int qsim_apply_pauli_sum(qsim_chunk* dst, const qsim_chunk* src, int n_terms, const uint64_t* x_masks, const uint64_t* z_masks,
                         const double* coeffs, int* n_passes) {
  const char* const what = "qsim_apply_pauli_sum";
  int rc = check_two_chunks(dst, src, n_terms, x_masks, z_masks, coeffs, true, coeffs, n_passes, what);
  if (rc) return rc;
  if (dst->amp < src->amp + amps(src) && src->amp < dst->amp + amps(dst))
    return fail(QSIM_ERR_INVALID, "%s: dst and src overlap (the call is out of place)", what);
  const int k = dst->k;
  PauliPasses pp;
  if ((rc = pauli_passes(k, n_terms, x_masks, z_masks, coeffs, &pp))) return rc;
  *n_passes = 0;
  HIP_TRY(hipSetDevice(dst->device));
  if (n_terms == 0) {
    hipLaunchKernelGGL(k_fill_zero, dim3(stream_grid(amps(dst))), dim3(kBlock), 0, dst->stream, dst->amp, amps(dst), 0);
    HIP_TRY(hipGetLastError());
    return QSIM_OK;
  }
  if ((rc = ensure_work(dst, sizeof(PauliTerm) * (u64)n_terms))) return rc;
  PauliTerm* dev_table = static_cast<PauliTerm*>(dst->work);
  HIP_TRY(hipMemcpyAsync(dev_table, pp.table.data(), sizeof(PauliTerm) * pp.table.size(), hipMemcpyHostToDevice, dst->stream));
  const bool nt = pair_streams(dst, src);
  const int np = (int)pp.plan.tile.size();
  for (int q = 0; q < np; ++q) {
    const bool acc = q > 0;
    const double bytes = (acc ? 48.0 : 32.0) * (double)amps(dst);
    ProfileScope prof(13, bytes, dst->stream, nt);
    if (pp.wide_term[(size_t)q] >= 0) {
      const int t = pp.wide_term[(size_t)q];
      PsumWideArgs w;
      std::memset(&w, 0, sizeof w);
      w.dst = dst->amp;
      w.src = src->amp;
      w.n = amps(dst);
      w.x = x_masks[t];
      w.z = z_masks[t];
      w.gr = pp.table[(size_t)pp.first[(size_t)q]].gr;
      w.gi = pp.table[(size_t)pp.first[(size_t)q]].gi;
      const unsigned grid = (unsigned)std::min<u64>(std::max<u64>(w.n / kBlock, 1), kExpMaxWg);
      if (acc) QSIM_WITH_NT(hipLaunchKernelGGL((k_psum_wide<NT, true>), dim3(grid), dim3(kBlock), 0, dst->stream, w));
      else QSIM_WITH_NT(hipLaunchKernelGGL((k_psum_wide<NT, false>), dim3(grid), dim3(kBlock), 0, dst->stream, w));
    } else {
      PsumArgs a;
      std::memset(&a, 0, sizeof a);
      a.dst = dst->amp;
      a.src = src->amp;
      a.terms = dev_table + pp.first[(size_t)q];
      pauli_tile_walk(k, pp.plan.tile[(size_t)q], &a);
      a.n_terms = pp.plan.count[(size_t)q];
      const unsigned grid = (unsigned)std::min<u64>(a.n_tiles, kExpMaxWg);
      if (acc) QSIM_WITH_NT(hipLaunchKernelGGL((k_psum_tile<NT, true>), dim3(grid), dim3(kBlock), 0, dst->stream, a));
      else QSIM_WITH_NT(hipLaunchKernelGGL((k_psum_tile<NT, false>), dim3(grid), dim3(kBlock), 0, dst->stream, a));
    }
    HIP_TRY(hipGetLastError());
    prof.done(dst->stream);
  }
  *n_passes = np;
  return QSIM_OK;
}

// The same plan; per pass k_ovl_tile (or k_ovl_wide) and k_hist_sum (the workgroup rows in workgroup order) into a
// device array of per-term (re, im), in pass order; one copy of 2 * n_terms doubles to the host at the end.  In the
// ket's workspace: the partials | the term table | the results.
int qsim_overlap_pauli(qsim_chunk* ket, const qsim_chunk* bra, int n_terms, const uint64_t* x_masks, const uint64_t* z_masks,
                       double* out_re_im, int* n_passes) {
  const char* const what = "qsim_overlap_pauli";
  int rc = check_two_chunks(ket, bra, n_terms, x_masks, z_masks, nullptr, false, out_re_im, n_passes, what);
  if (rc) return rc;
  const int k = ket->k;
  PauliPasses pp;
  if ((rc = pauli_passes(k, n_terms, x_masks, z_masks, nullptr, &pp))) return rc;
  *n_passes = 0;
  if (n_terms == 0) return QSIM_OK;
  const int np = (int)pp.plan.tile.size();
  int max_count = 1;
  for (int q = 0; q < np; ++q) max_count = std::max(max_count, pp.plan.count[(size_t)q]);
  // (a wide pass has up to kExpMaxWg rows of 2 doubles, a tile pass up to kOvlMaxWg rows of 2 * count)
  const u64 partial_bytes = sizeof(double) * 2 * std::max<u64>((u64)kOvlMaxWg * (u64)max_count, kExpMaxWg);
  const u64 table_off = partial_bytes, out_off = table_off + sizeof(PauliTerm) * (u64)n_terms;
  if ((rc = ensure_work(ket, out_off + sizeof(double) * 2 * (u64)n_terms))) return rc;
  char* base = static_cast<char*>(ket->work);
  double* partial = reinterpret_cast<double*>(base);
  PauliTerm* dev_table = reinterpret_cast<PauliTerm*>(base + table_off);
  double* dev_out = reinterpret_cast<double*>(base + out_off);
  HIP_TRY(hipSetDevice(ket->device));
  HIP_TRY(hipMemcpyAsync(dev_table, pp.table.data(), sizeof(PauliTerm) * pp.table.size(), hipMemcpyHostToDevice, ket->stream));
  const bool nt = pair_streams(ket, bra);
  const double bytes = 32.0 * (double)amps(ket);
  for (int q = 0; q < np; ++q) {
    const int first = pp.first[(size_t)q];
    unsigned grid;
    int width;
    {
      ProfileScope prof(14, bytes, ket->stream, nt);
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
        w.gr = pp.table[(size_t)first].gr;
        w.gi = pp.table[(size_t)first].gi;
        grid = (unsigned)std::min<u64>(std::max<u64>(w.n / kBlock, 1), kExpMaxWg);
        width = 2;
        QSIM_WITH_NT(hipLaunchKernelGGL((k_ovl_wide<NT>), dim3(grid), dim3(kBlock), 0, ket->stream, w));
      } else {
        OvlArgs a;
        std::memset(&a, 0, sizeof a);
        a.bra = bra->amp;
        a.ket = ket->amp;
        a.terms = dev_table + first;
        a.partial = partial;
        pauli_tile_walk(k, pp.plan.tile[(size_t)q], &a);
        a.n_terms = pp.plan.count[(size_t)q];
        int slices = 1;
        while (slices * 2 * a.n_terms <= kBlock) slices *= 2;
        a.slices = slices;
        grid = (unsigned)std::min<u64>(a.n_tiles, kOvlMaxWg);
        width = 2 * a.n_terms;
        QSIM_WITH_NT(hipLaunchKernelGGL((k_ovl_tile<NT>), dim3(grid), dim3(kBlock), 0, ket->stream, a));
      }
      HIP_TRY(hipGetLastError());
      prof.done(ket->stream);
    }
    if ((rc = sum_rows(ket, partial, grid, width, dev_out + 2 * first))) return rc;
  }
  std::vector<double> res(2 * (size_t)n_terms);
  if ((rc = fetch_doubles(ket, dev_out, 2 * (u64)n_terms, res.data()))) return rc;
  for (int t = 0; t < n_terms; ++t) {
    out_re_im[2 * t] = res[2 * (size_t)pp.slot[(size_t)t]];
    out_re_im[2 * t + 1] = res[2 * (size_t)pp.slot[(size_t)t] + 1];
  }
  *n_passes = np;
  return QSIM_OK;
}
}  // extern "C"
