// abi_lincomb.h -- C ABI: vector algebra on whole chunks: a linear combination with the inner products and the norm of
// the result taken in the same pass (lincomb_kernels.h).
// Part of the single translation unit qsim_hip.hip (included there, in order; not a standalone header).
// The argument checks are the pair checks of check_pauli_call (abi_readout.h), made for dst against every other chunk.

// Do the distinct allocations behind the chunks together exceed the Infinity Cache?  (pair_streams for a list: views
// of one parent, and handles on the same memory, share an allocation.)
static bool list_streams(const qsim_chunk* const* cs, int n) {
  u64 bytes = 0;
  for (int i = 0; i < n; ++i) {
    bool seen = false;
    for (int j = 0; j < i && !seen; ++j)
      seen = cs[i]->amp == cs[j]->amp || (cs[i]->parent && cs[i]->parent == cs[j]->parent) || cs[i]->parent == cs[j] || cs[j]->parent == cs[i];
    if (!seen) bytes += cs[i]->span_bytes;
  }
  return bytes > tuning().mall_bytes;
}

extern "C" {
int qsim_lincomb(qsim_chunk* dst, const double dst_coeff[2], int n_src, const qsim_chunk* const* srcs, const double* coeffs_re_im,
                 int n_bras, const qsim_chunk* const* bras, double* dots_re_im, double* norm2) {
  const char* const what = "qsim_lincomb";
  int rc = check_chunk(dst, what);
  if (rc) return rc;
  if (n_src < 0 || n_src > kLcMaxStreams) return fail(QSIM_ERR_INVALID, "%s: 0 <= n_src <= %d expected, got %d", what, kLcMaxStreams, n_src);
  if (n_bras < 0 || n_bras > kLcMaxStreams) return fail(QSIM_ERR_INVALID, "%s: 0 <= n_bras <= %d expected, got %d", what, kLcMaxStreams, n_bras);
  if (!dst_coeff || (n_src > 0 && (!srcs || !coeffs_re_im)) || (n_bras > 0 && (!bras || !dots_re_im)))
    return fail(QSIM_ERR_INVALID, "%s: null argument", what);
  const qsim_chunk* all[1 + 2 * kLcMaxStreams] = {dst};
  int n_all = 1;
  for (int s = 0; s < n_src; ++s) all[n_all++] = srcs[s];
  for (int b = 0; b < n_bras; ++b) all[n_all++] = bras[b];
  for (int i = 1; i < n_all; ++i)
    if ((rc = check_chunk(all[i], what))) return rc;
  if (!std::isfinite(dst_coeff[0]) || !std::isfinite(dst_coeff[1])) return fail(QSIM_ERR_INVALID, "%s: dst_coeff is not finite", what);
  for (int s = 0; s < n_src; ++s)
    if (!std::isfinite(coeffs_re_im[2 * s]) || !std::isfinite(coeffs_re_im[2 * s + 1]))
      return fail(QSIM_ERR_INVALID, "%s: coefficient of source %d is not finite", what, s);
  for (int i = 1; i < n_all; ++i)
    if ((rc = check_two_chunks(dst, all[i], what))) return rc;
  for (int i = 0; i < n_all; ++i)
    if ((rc = require_no_parts(all[i], what))) return rc;
  for (int i = 1; i < n_all; ++i)
    if (dst->amp < all[i]->amp + amps(all[i]) && all[i]->amp < dst->amp + amps(dst))
      return fail(QSIM_ERR_INVALID, "%s: %s %d and dst overlap (sources and bras are only read, dst is updated in place)", what,
                  i <= n_src ? "source" : "bra", i <= n_src ? i - 1 : i - 1 - n_src);

  const bool rd = !(dst_coeff[0] == 0.0 && dst_coeff[1] == 0.0);
  const bool wr = !(n_src == 0 && dst_coeff[0] == 1.0 && dst_coeff[1] == 0.0);
  LincombArgs a;
  std::memset(&a, 0, sizeof a);
  a.dst = dst->amp;
  a.cd = make_double2(dst_coeff[0], dst_coeff[1]);
  for (int s = 0; s < n_src; ++s) {
    a.src[s] = srcs[s]->amp;
    a.cs[s] = make_double2(coeffs_re_im[2 * s], coeffs_re_im[2 * s + 1]);
  }
  // A bra on the memory of a source (or of an earlier bra) is not loaded again: col_of[b] = the column pair it shares.
  int nb = 0, n_cols = 0, col_of[kLcMaxStreams];
  int slot_of_pair[2 * kLcMaxStreams];              // column pair -> first value slot of the kernel
  for (int b = 0; b < n_bras; ++b) {
    int slot = -1;
    for (int s = 0; s < n_src && slot < 0; ++s) if (bras[b]->amp == srcs[s]->amp) slot = 2 * s;
    for (int j = 0; j < nb && slot < 0; ++j) if (bras[b]->amp == a.bra[j]) slot = 2 * n_src + 2 * j;
    if (slot < 0) {
      a.bra[nb] = bras[b]->amp;
      slot = 2 * n_src + 2 * nb++;
    }
    if (slot < 2 * n_src) a.src_dot |= 1 << (slot >> 1);
    col_of[b] = -1;
    for (int c = 0; c < n_cols; ++c) if (slot_of_pair[c] == slot) col_of[b] = c;
    if (col_of[b] < 0) { slot_of_pair[n_cols] = slot; col_of[b] = n_cols++; }
  }
  for (int c = 0; c < n_cols; ++c) {
    a.slot_of_col[2 * c] = (signed char)slot_of_pair[c];
    a.slot_of_col[2 * c + 1] = (signed char)(slot_of_pair[c] + 1);
  }
  a.width = 2 * n_cols;
  if (norm2) {
    a.want_norm = 1;
    a.slot_of_col[a.width++] = (signed char)(kLcSlots - 1);
  }
  if (!wr && a.width == 0) return QSIM_OK;          // nothing to write and nothing to reduce: no launch
  a.n = amps(dst);
  // The grid is bounded where there are partial rows to bound; a call that reduces nothing runs one workgroup per block
  // like k_copy (the looped form costs a written pass 10-15 %: profiles/r21_lincomb_ab.json).
  int items = kLcItems;
  unsigned max_wg = a.width ? kLcMaxWg : kMaxGridX;
#ifdef QSIM_PROBES
  // Probe build only, read at EVERY call so that one process compares settings on the same buffers (tools/krylov_probe.py
  // --ab): QSIM_LC_ITEMS=2 (two amplitudes per thread and block), QSIM_LC_MAX_WG (the grid cap of every form, a multiple of 8).
  if (const char* e = getenv("QSIM_LC_ITEMS")) items = atoi(e) == 2 ? 2 : kLcItems;
  if (const char* e = getenv("QSIM_LC_MAX_WG")) max_wg = std::max(8u, std::min((unsigned)atoi(e), kMaxGridX) & ~7u);
#endif
  a.blocks = (a.n + (u64)(kBlock * items) - 1) / (u64)(kBlock * items);
  const unsigned grid = (unsigned)std::min<u64>(a.blocks, max_wg);
  double* dev_out = nullptr;
  if (a.width) {
    if ((rc = ensure_work(dst, sizeof(double) * ((u64)grid + 1) * (u64)a.width))) return rc;
    a.partial = static_cast<double*>(dst->work);
    dev_out = a.partial + (u64)grid * a.width;
  }
  HIP_TRY(hipSetDevice(dst->device));
  bool nt = list_streams(all, n_all);
#ifdef QSIM_PROBES
  if (tuning().force_nt >= 0) nt = tuning().force_nt != 0;
#endif
  {
    const double bytes = 16.0 * (double)((rd ? 1 : 0) + n_src + nb + (wr ? 1 : 0)) * (double)a.n;
    ProfileScope prof(kClsLincomb, bytes, dst->stream, nt);
#ifdef QSIM_PROBES
    if (items == 2) QSIM_WITH_NT((launch_lincomb<NT, 2>(rd, wr, n_src, nb, grid, dst->stream, a)));
    else
#endif
    QSIM_WITH_NT(launch_lincomb<NT>(rd, wr, n_src, nb, grid, dst->stream, a));
  }
  HIP_TRY(hipGetLastError());
  if (!a.width) return QSIM_OK;                     // enqueued on dst's stream like the gate calls
  if ((rc = sum_rows(dst, a.partial, grid, a.width, dev_out))) return rc;
  double res[kLcMaxWidth];
  if ((rc = fetch_doubles(dst, dev_out, (u64)a.width, res))) return rc;
  for (int b = 0; b < n_bras; ++b) {
    dots_re_im[2 * b] = res[2 * col_of[b]];
    dots_re_im[2 * b + 1] = res[2 * col_of[b] + 1];
  }
  if (norm2) *norm2 = res[a.width - 1];
  return QSIM_OK;
}
}  // extern "C"
