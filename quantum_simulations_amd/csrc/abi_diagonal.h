// abi_diagonal.h -- C ABI: diagonal Pauli sums D = sum_t c_t Z^{z_t} on a chunk: the phase exp(-i gamma D) in place, the
// moments sum |psi|^2 (1, E, E^2) read-only, and D as an operator between two chunks, dst (+)= D src and <bra|D|ket>,
// each ONE pass whatever the number of terms, and the values of the single terms <Z^{z_t}>, one read-only pass per 2048
// terms (diag_kernels.h).
// Part of the single translation unit qsim_hip.hip (included there, in order; not a standalone header).

// What the four calls share: the checks (the chunk, then check_diag_args, then pending parts; with a second chunk
// `other`, then that chunk, the pair checks of check_two_chunks and its pending parts), the tables of diag_plan.h
// as one block in the chunk's workspace -- terms | pieces | joins, 16-byte records, then `extra` bytes for the caller --
// and the launch arguments.  The block is copied from a vector of this call (hipMemcpyAsync from host memory that is
// not pinned copies before it returns, as in qsim_apply_pauli_rotations).
static int diag_prepare(qsim_chunk* c, const qsim_chunk* other, int n_terms, const uint64_t* z_masks, const double* coeffs,
                        const double* gamma, u64 extra, const char* what, DiagArgs* a, char** extra_at) {
  int rc = check_chunk(c, what);
  if (rc || (rc = check_diag_args(c->k, n_terms, z_masks, coeffs, gamma, what)) || (rc = require_no_parts(c, what))) return rc;
  if (other && ((rc = check_chunk(other, what)) || (rc = check_two_chunks(c, other, what)) || (rc = require_no_parts(other, what)))) return rc;
  std::memset(a, 0, sizeof *a);
  a->amp = c->amp;
  a->other = other ? other->amp : nullptr;
  a->tb = std::min(c->k, kExpTileBits);
  a->n_tiles = 1ull << (c->k - a->tb);
  if (n_terms == 0 && extra == 0) return QSIM_OK;   // (nothing will be launched)
  DiagTable d;
  diag_table(a->tb, n_terms, z_masks, coeffs, &d);
  if (d.n_slots > kDiagMaxSlots) return fail(QSIM_ERR_INVALID, "internal: %s needs %d piece slots", what, d.n_slots);
  static_assert(sizeof(DiagTerm) == 16 && sizeof(DiagPiece) == 16 && sizeof(DiagJoin) == 16, "16-byte records");
  const u64 piece_off = 16 * d.terms.size(), join_off = piece_off + 16 * d.pieces.size(), extra_off = join_off + 16 * d.joins.size();
  if ((rc = ensure_work(c, extra_off + extra))) return rc;
  char* const base = static_cast<char*>(c->work);
  HIP_TRY(hipSetDevice(c->device));
  if (extra_off) {
    std::vector<char> block((size_t)extra_off);
    if (piece_off) std::memcpy(block.data(), d.terms.data(), (size_t)piece_off);
    if (join_off > piece_off) std::memcpy(block.data() + piece_off, d.pieces.data(), (size_t)(join_off - piece_off));
    if (extra_off > join_off) std::memcpy(block.data() + join_off, d.joins.data(), (size_t)(extra_off - join_off));
    HIP_TRY(hipMemcpyAsync(base, block.data(), (size_t)extra_off, hipMemcpyHostToDevice, c->stream));
  }
  a->terms = reinterpret_cast<const DiagTerm*>(base);
  a->pieces = reinterpret_cast<const DiagPiece*>(base + piece_off);
  a->joins = reinterpret_cast<const DiagJoin*>(base + join_off);
  a->n_pieces = (int)d.pieces.size();
  a->n_joins = (int)d.joins.size();
  *extra_at = base + extra_off;
  return QSIM_OK;
}

extern "C" {
int qsim_apply_diagonal_phase(qsim_chunk* c, int n_terms, const uint64_t* z_masks, const double* coeffs, double gamma) {
  DiagArgs a;
  char* extra = nullptr;
  int rc = diag_prepare(c, nullptr, n_terms, z_masks, coeffs, &gamma, 0, "qsim_apply_diagonal_phase", &a, &extra);
  if (rc || n_terms == 0) return rc;
  a.gamma = gamma;
  const bool nt = c->span_bytes > tuning().mall_bytes;
  const unsigned grid = (unsigned)std::min<u64>(a.n_tiles, kExpMaxWg);
  ProfileScope prof(16, 32.0 * (double)amps(c), c->stream, nt);
  QSIM_WITH_NT(hipLaunchKernelGGL((k_diag_tile<NT, kDiagPhase>), dim3(grid), dim3(kBlock), 0, c->stream, a));
  HIP_TRY(hipGetLastError());
  prof.done(c->stream);
  return QSIM_OK;
}

int qsim_diagonal_moments(qsim_chunk* c, int n_terms, const uint64_t* z_masks, const double* coeffs, double out[3]) {
  const char* const what = "qsim_diagonal_moments";
  int rc = check_chunk(c, what);
  if (rc) return rc;
  if (!out) return fail(QSIM_ERR_INVALID, "%s: null argument", what);
  DiagArgs a;
  char* extra = nullptr;
  const unsigned max_grid = kExpMaxWg;
  if ((rc = diag_prepare(c, nullptr, n_terms, z_masks, coeffs, nullptr, sizeof(double) * 3 * ((u64)max_grid + 1), what, &a, &extra))) return rc;
  const unsigned grid = (unsigned)std::min<u64>(a.n_tiles, max_grid);
  a.partial = reinterpret_cast<double*>(extra);
  double* const dev_out = a.partial + 3 * (u64)grid;
  const bool nt = c->span_bytes > tuning().mall_bytes;
  {
    ProfileScope prof(16, 16.0 * (double)amps(c), c->stream, nt);
    QSIM_WITH_NT(hipLaunchKernelGGL((k_diag_tile<NT, kDiagMoments>), dim3(grid), dim3(kBlock), 0, c->stream, a));
    HIP_TRY(hipGetLastError());
    prof.done(c->stream);
  }
  if ((rc = sum_rows(c, a.partial, grid, 3, dev_out))) return rc;
  return fetch_doubles(c, dev_out, 3, out);
}

// dst = D src (accumulate 0) or dst += D src (1), one pass on dst's stream, not waited for; the tables in dst's workspace.
int qsim_apply_diagonal_sum(qsim_chunk* dst, const qsim_chunk* src, int n_terms, const uint64_t* z_masks, const double* coeffs,
                            int accumulate) {
  const char* const what = "qsim_apply_diagonal_sum";
  int rc = check_chunk(dst, what);
  if (rc || (rc = check_chunk(src, what))) return rc;
  if (accumulate != 0 && accumulate != 1) return fail(QSIM_ERR_INVALID, "%s: accumulate = %d, 0 or 1 expected", what, accumulate);
  if (dst->amp < src->amp + amps(src) && src->amp < dst->amp + amps(dst) && (dst->amp != src->amp || dst->k != src->k || accumulate))
    return fail(QSIM_ERR_INVALID, "%s: dst and src overlap (only dst = D dst over the same range, without accumulate, is in place)", what);
  DiagArgs a;
  char* extra = nullptr;
  if ((rc = diag_prepare(dst, src, n_terms, z_masks, coeffs, nullptr, 0, what, &a, &extra))) return rc;
  if (n_terms == 0) {
    if (accumulate) return QSIM_OK;
    HIP_TRY(hipSetDevice(dst->device));
    hipLaunchKernelGGL(k_fill_zero, dim3(stream_grid(amps(dst))), dim3(kBlock), 0, dst->stream, dst->amp, amps(dst), 0);
    HIP_TRY(hipGetLastError());
    return QSIM_OK;
  }
  std::swap(a.amp, a.other);                        // the kernel loads a.amp = src first and writes a.other = dst
  const bool nt = pair_streams(dst, src);
  const unsigned grid = (unsigned)std::min<u64>(a.n_tiles, kExpMaxWg);
  ProfileScope prof(17, (accumulate ? 48.0 : 32.0) * (double)amps(dst), dst->stream, nt);
  if (accumulate) QSIM_WITH_NT(hipLaunchKernelGGL((k_diag_apply<NT, true>), dim3(grid), dim3(kBlock), 0, dst->stream, a));
  else QSIM_WITH_NT(hipLaunchKernelGGL((k_diag_apply<NT, false>), dim3(grid), dim3(kBlock), 0, dst->stream, a));
  HIP_TRY(hipGetLastError());
  prof.done(dst->stream);
  return QSIM_OK;
}

// out = (re, im of <bra|ket>, re, im of <bra|D|ket>): one read-only pass, the tables and the partial rows in ket's workspace.
int qsim_overlap_diagonal(qsim_chunk* ket, const qsim_chunk* bra, int n_terms, const uint64_t* z_masks, const double* coeffs,
                          double out[4]) {
  const char* const what = "qsim_overlap_diagonal";
  int rc = check_chunk(ket, what);
  if (rc || (rc = check_chunk(bra, what))) return rc;
  if (!out) return fail(QSIM_ERR_INVALID, "%s: null argument", what);
  DiagArgs a;
  char* extra = nullptr;
  const unsigned max_grid = kExpMaxWg;
  if ((rc = diag_prepare(ket, bra, n_terms, z_masks, coeffs, nullptr, sizeof(double) * 4 * ((u64)max_grid + 1), what, &a, &extra))) return rc;
  const unsigned grid = (unsigned)std::min<u64>(a.n_tiles, max_grid);
  a.partial = reinterpret_cast<double*>(extra);
  double* const dev_out = a.partial + 4 * (u64)grid;
  const bool nt = pair_streams(ket, bra);
  {
    ProfileScope prof(18, 32.0 * (double)amps(ket), ket->stream, nt);
    QSIM_WITH_NT(hipLaunchKernelGGL((k_diag_overlap<NT>), dim3(grid), dim3(kBlock), 0, ket->stream, a));
    HIP_TRY(hipGetLastError());
    prof.done(ket->stream);
  }
  if ((rc = sum_rows(ket, a.partial, grid, 4, dev_out))) return rc;
  return fetch_doubles(ket, dev_out, 4, out);
}

// out[t] = sum_i |psi_i|^2 (-1)^popcount(i & z_masks[t]), in input order: one read-only pass per kDiagValuesPerPass
// terms.  The workspace holds the records of the whole list | the n_terms sums | the rows of ONE pass, [workgroup][terms
// of the pass]: the passes run one after the other on the chunk's stream and share the rows; the sums cross once.
int qsim_expectation_z_terms(qsim_chunk* c, int n_terms, const uint64_t* z_masks, double* out, int* n_passes) {
  const char* const what = "qsim_expectation_z_terms";
  int rc = check_chunk(c, what);
  if (rc || (rc = check_diag_value_args(c->k, n_terms, z_masks, out, what)) || (rc = require_no_parts(c, what))) return rc;
  if (n_passes) *n_passes = 0;
  if (n_terms == 0) return QSIM_OK;
  DiagValueArgs a;
  std::memset(&a, 0, sizeof a);
  a.amp = c->amp;
  a.tb = std::min(c->k, kExpTileBits);
  a.n_tiles = 1ull << (c->k - a.tb);
  DiagValueTable d;
  diag_value_table(a.tb, n_terms, z_masks, &d);
  static_assert(sizeof(DiagValueTerm) == 16, "16-byte records");
  const unsigned grid = (unsigned)std::min<u64>(a.n_tiles, kExpMaxWg);
  const u64 out_off = 16 * (u64)n_terms, row_off = out_off + 8 * (u64)n_terms;
  if ((rc = ensure_work(c, row_off + 8 * (u64)grid * (u64)std::min(n_terms, kDiagValuesPerPass)))) return rc;
  char* const base = static_cast<char*>(c->work);
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemcpyAsync(base, d.terms.data(), (size_t)out_off, hipMemcpyHostToDevice, c->stream));
  double* const dev_out = reinterpret_cast<double*>(base + out_off);
  a.partial = reinterpret_cast<double*>(base + row_off);
  const bool nt = c->span_bytes > tuning().mall_bytes;
  for (const DiagValuePass& p : d.passes) {
    a.terms = reinterpret_cast<const DiagValueTerm*>(base) + p.first;
    a.n_terms = p.count;
    {
      ProfileScope prof(19, 16.0 * (double)amps(c), c->stream, nt);
      QSIM_WITH_NT(hipLaunchKernelGGL((k_diag_term_values<NT>), dim3(grid), dim3(kBlock), 0, c->stream, a));
      HIP_TRY(hipGetLastError());
      prof.done(c->stream);
    }
    if ((rc = sum_rows(c, a.partial, grid, p.count, dev_out + p.first))) return rc;
  }
  if (n_passes) *n_passes = (int)d.passes.size();
  return fetch_doubles(c, dev_out, (u64)n_terms, out);
}
}  // extern "C"
