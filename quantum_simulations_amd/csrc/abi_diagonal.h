// abi_diagonal.h -- C ABI: diagonal Pauli sums D = sum_t c_t Z^{z_t} on a chunk: the phase exp(-i gamma D) in place, the
// moments sum |psi|^2 (1, E, E^2) read-only, and D as an operator between two chunks, dst (+)= D src and <bra|D|ket>,
// each ONE pass whatever the number of terms, and the values of the single terms <Z^{z_t}>, one read-only pass per 2048
// terms (diag_kernels.h).
// Part of the single translation unit qsim_hip.hip (included there, in order; not a standalone header).

// The tile geometry of a chunk of k index bits, for all five calls: contiguous tiles of tb bits, one workgroup per tile
// up to kExpMaxWg workgroups, which then loop.
struct DiagGeom {
  int tb;                // tile bits: min(k, kExpTileBits)
  u64 n_tiles;           // 2^(k - tb)
  unsigned grid;
};
static DiagGeom diag_geom(int k) {
  const int tb = std::min(k, kExpTileBits);
  const u64 n_tiles = 1ull << (k - tb);
  return {tb, n_tiles, (unsigned)std::min<u64>(n_tiles, kExpMaxWg)};
}

// What the four calls with coefficients share: the checks (the chunk, then check_diag_args, then pending parts; with a
// second chunk `other`, then that chunk, the pair checks of check_two_chunks and its pending parts), the tables of
// diag_plan.h as one block in the chunk's workspace -- terms | pieces | joins, 16-byte records, then for a reducing call
// a->partial: kExpMaxWg rows of `width` doubles and the result (diag_reduce) -- and the launch arguments.  The block is
// copied from a vector of this call (hipMemcpyAsync from host memory that is not pinned copies before it returns, as in
// qsim_apply_pauli_rotations).
static int diag_prepare(qsim_chunk* c, const qsim_chunk* other, int n_terms, const uint64_t* z_masks, const double* coeffs,
                        const double* gamma, int width, const char* what, DiagArgs* a, DiagGeom* g) {
  int rc = check_chunk(c, what);
  if (rc || (rc = check_diag_args(c->k, n_terms, z_masks, coeffs, true, gamma, what)) || (rc = require_no_parts(c, what))) return rc;
  if (other && ((rc = check_chunk(other, what)) || (rc = check_two_chunks(c, other, what)) || (rc = require_no_parts(other, what)))) return rc;
  *g = diag_geom(c->k);
  std::memset(a, 0, sizeof *a);
  a->amp = c->amp;
  a->other = other ? other->amp : nullptr;
  a->tb = g->tb;
  a->n_tiles = g->n_tiles;
  if (n_terms == 0 && width == 0) return QSIM_OK;   // (nothing will be launched)
  DiagTable d;
  diag_table(a->tb, n_terms, z_masks, coeffs, &d);
  if (d.n_slots > kDiagMaxSlots) return fail(QSIM_ERR_INVALID, "internal: %s needs %d piece slots", what, d.n_slots);
  static_assert(sizeof(DiagTerm) == 16 && sizeof(DiagPiece) == 16 && sizeof(DiagJoin) == 16, "16-byte records");
  const u64 piece_off = 16 * d.terms.size(), join_off = piece_off + 16 * d.pieces.size(), extra_off = join_off + 16 * d.joins.size();
  if ((rc = ensure_work(c, extra_off + sizeof(double) * (u64)width * ((u64)kExpMaxWg + 1)))) return rc;
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
  a->partial = reinterpret_cast<double*>(base + extra_off);
  return QSIM_OK;
}

// A launch under the profile: launch() starts the kernel on c's stream, the scope closes before anything else is queued.
template <class Launch>
static int diag_launch(qsim_chunk* c, KernelClass cls, double bytes, bool nt, Launch launch) {
  {
    ProfileScope prof(cls, bytes, c->stream, nt);
    launch();
  }
  HIP_TRY(hipGetLastError());
  return QSIM_OK;
}

// The finish of moments (width 3) and overlap (width 4), rows | result at `rows` (diag_prepare's a->partial): the launch,
// whose g.grid workgroups each write a row of `width` doubles, k_hist_sum over the rows in workgroup order, and the
// `width` results on the host when it returns.
template <class Launch>
static int diag_reduce(qsim_chunk* c, KernelClass cls, double bytes, bool nt, const DiagGeom& g, int width, double* rows, double* out,
                       Launch launch) {
  double* const dev_out = rows + (u64)width * g.grid;
  int rc = diag_launch(c, cls, bytes, nt, launch);
  if (rc || (rc = sum_rows(c, rows, g.grid, width, dev_out))) return rc;
  return fetch_doubles(c, dev_out, (u64)width, out);
}

extern "C" {
int qsim_apply_diagonal_phase(qsim_chunk* c, int n_terms, const uint64_t* z_masks, const double* coeffs, double gamma) {
  DiagArgs a;
  DiagGeom g;
  int rc = diag_prepare(c, nullptr, n_terms, z_masks, coeffs, &gamma, 0, "qsim_apply_diagonal_phase", &a, &g);
  if (rc || n_terms == 0) return rc;
  a.gamma = gamma;
  const bool nt = c->span_bytes > tuning().mall_bytes;
  return diag_launch(c, kClsDiag, 32.0 * (double)amps(c), nt, [&] {
    QSIM_WITH_NT(hipLaunchKernelGGL((k_diag_tile<NT, kDiagPhase>), dim3(g.grid), dim3(kBlock), 0, c->stream, a));
  });
}

int qsim_diagonal_moments(qsim_chunk* c, int n_terms, const uint64_t* z_masks, const double* coeffs, double out[3]) {
  const char* const what = "qsim_diagonal_moments";
  int rc = check_chunk(c, what);
  if (rc) return rc;
  if (!out) return fail(QSIM_ERR_INVALID, "%s: null argument", what);
  DiagArgs a;
  DiagGeom g;
  if ((rc = diag_prepare(c, nullptr, n_terms, z_masks, coeffs, nullptr, 3, what, &a, &g))) return rc;
  const bool nt = c->span_bytes > tuning().mall_bytes;
  return diag_reduce(c, kClsDiag, 16.0 * (double)amps(c), nt, g, 3, a.partial, out, [&] {
    QSIM_WITH_NT(hipLaunchKernelGGL((k_diag_tile<NT, kDiagMoments>), dim3(g.grid), dim3(kBlock), 0, c->stream, a));
  });
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
  DiagGeom g;
  if ((rc = diag_prepare(dst, src, n_terms, z_masks, coeffs, nullptr, 0, what, &a, &g))) return rc;
  if (n_terms == 0) {
    if (accumulate) return QSIM_OK;
    HIP_TRY(hipSetDevice(dst->device));
    hipLaunchKernelGGL(k_fill_zero, dim3(stream_grid(amps(dst))), dim3(kBlock), 0, dst->stream, dst->amp, amps(dst), 0);
    HIP_TRY(hipGetLastError());
    return QSIM_OK;
  }
  std::swap(a.amp, a.other);                        // the kernel loads a.amp = src first and writes a.other = dst
  const bool nt = pair_streams(dst, src);
  return diag_launch(dst, kClsDiagApply, (accumulate ? 48.0 : 32.0) * (double)amps(dst), nt, [&] {
    if (accumulate) QSIM_WITH_NT(hipLaunchKernelGGL((k_diag_apply<NT, true>), dim3(g.grid), dim3(kBlock), 0, dst->stream, a));
    else QSIM_WITH_NT(hipLaunchKernelGGL((k_diag_apply<NT, false>), dim3(g.grid), dim3(kBlock), 0, dst->stream, a));
  });
}

// out = (re, im of <bra|ket>, re, im of <bra|D|ket>): one read-only pass, the tables and the partial rows in ket's workspace.
int qsim_overlap_diagonal(qsim_chunk* ket, const qsim_chunk* bra, int n_terms, const uint64_t* z_masks, const double* coeffs,
                          double out[4]) {
  const char* const what = "qsim_overlap_diagonal";
  int rc = check_chunk(ket, what);
  if (rc || (rc = check_chunk(bra, what))) return rc;
  if (!out) return fail(QSIM_ERR_INVALID, "%s: null argument", what);
  DiagArgs a;
  DiagGeom g;
  if ((rc = diag_prepare(ket, bra, n_terms, z_masks, coeffs, nullptr, 4, what, &a, &g))) return rc;
  const bool nt = pair_streams(ket, bra);
  return diag_reduce(ket, kClsDiagOverlap, 32.0 * (double)amps(ket), nt, g, 4, a.partial, out, [&] {
    QSIM_WITH_NT(hipLaunchKernelGGL((k_diag_overlap<NT>), dim3(g.grid), dim3(kBlock), 0, ket->stream, a));
  });
}

// out[t] = sum_i |psi_i|^2 (-1)^popcount(i & z_masks[t]), in input order: one read-only pass per kDiagValuesPerPass
// terms.  The workspace holds the records of the whole list | the n_terms sums | the rows of ONE pass, [workgroup][terms
// of the pass]: the passes run one after the other on the chunk's stream and share the rows; the sums cross once.
int qsim_expectation_z_terms(qsim_chunk* c, int n_terms, const uint64_t* z_masks, double* out, int* n_passes) {
  const char* const what = "qsim_expectation_z_terms";
  int rc = check_chunk(c, what);
  if (rc || (rc = check_diag_args(c->k, n_terms, z_masks, out, false, nullptr, what)) || (rc = require_no_parts(c, what))) return rc;
  if (n_passes) *n_passes = 0;
  if (n_terms == 0) return QSIM_OK;
  const DiagGeom g = diag_geom(c->k);
  DiagValueArgs a;
  std::memset(&a, 0, sizeof a);
  a.amp = c->amp;
  a.tb = g.tb;
  a.n_tiles = g.n_tiles;
  DiagValueTable d;
  diag_value_table(a.tb, n_terms, z_masks, &d);
  static_assert(sizeof(DiagValueTerm) == 16, "16-byte records");
  const u64 out_off = 16 * (u64)n_terms, row_off = out_off + 8 * (u64)n_terms;
  if ((rc = ensure_work(c, row_off + 8 * (u64)g.grid * (u64)std::min(n_terms, kDiagValuesPerPass)))) return rc;
  char* const base = static_cast<char*>(c->work);
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemcpyAsync(base, d.terms.data(), (size_t)out_off, hipMemcpyHostToDevice, c->stream));
  double* const dev_out = reinterpret_cast<double*>(base + out_off);
  a.partial = reinterpret_cast<double*>(base + row_off);
  const bool nt = c->span_bytes > tuning().mall_bytes;
  for (const DiagValuePass& p : d.passes) {
    a.terms = reinterpret_cast<const DiagValueTerm*>(base) + p.first;
    a.n_terms = p.count;
    rc = diag_launch(c, kClsDiagTermValues, 16.0 * (double)amps(c), nt, [&] {
      QSIM_WITH_NT(hipLaunchKernelGGL((k_diag_term_values<NT>), dim3(g.grid), dim3(kBlock), 0, c->stream, a));
    });
    if (rc || (rc = sum_rows(c, a.partial, g.grid, p.count, dev_out + p.first))) return rc;
  }
  if (n_passes) *n_passes = (int)d.passes.size();
  return fetch_doubles(c, dev_out, (u64)n_terms, out);
}
}  // extern "C"
