// diag_plan.h -- host side of the diagonal Pauli sums (diag_kernels.h, abi_diagonal.h): the argument checks and the
// tables k_diag_tile and k_diag_term_values read.  Pure C++, no device call and no HIP type: tools/diag_plan_check.cpp
// compiles this file alone, with stubs for fail() and the error codes, under the host sanitizers.
// Part of the single translation unit qsim_hip.hip (included there before diag_kernels.h; not a standalone header).
//
// D = sum_t c_t Z^{z_t}, z_t a mask of physical index bits (0: the identity).  A tile is the 2^tb amplitudes on the
// lowest tb = min(k, kExpTileBits) index bits; zi = z & (2^tb - 1) is the part of a mask inside the tile, zo the rest.
// The spectrum of a tile is W[m] = sum_{t: zi_t = m} c_t (-1)^popcount(base & zo_t), so the table is the terms SORTED
// BY zi (stable: ties stay in input order) and cut into segments of equal zi.  A segment of more than kDiagPiece terms
// is cut into pieces of kDiagPiece (the last one shorter); a thread sums one piece in table order, a single-piece
// segment goes straight into W, the pieces of a longer one into consecutive slots of an LDS array that one thread adds
// in piece order (a "join").  The order of every sum is a function of the term list and k alone: no grid size, no
// atomics, two calls give the same bits.
constexpr int kDiagMaxTerms = 16384;                // terms of one call
// terms one thread sums in a row.  Measured at 30 qubits with 16 / 32 / 64 (profiles/r22_diagonal_ab.json): shorter pieces
// spread a cost layer's few long segments over more threads (the 435 ZZ pairs: 7.25 / 7.40 / 8.14 ms), longer ones keep
// the join of one huge segment short (4096 masks on the high bits only: 12.5 / 11.1 / 10.4 ms)
constexpr int kDiagPiece = 32;
// slots of the pieces of multi-piece segments: a segment of L > kDiagPiece terms has ceil(L / kDiagPiece) <=
// L / kDiagPiece + 1 <= 2 L / kDiagPiece pieces
constexpr int kDiagMaxSlots = 2 * kDiagMaxTerms / kDiagPiece;

struct DiagTerm {        // 16 bytes, in table order
  u64 zo;                // z outside the tile (physical bits): the outer sign
  double c;
};
struct DiagPiece {       // 16 bytes
  int first, count;      // terms first .. first + count - 1 of the table, count <= kDiagPiece
  unsigned zi;           // the segment's spectrum index
  int slot;              // -1: the whole segment, the sum goes into W[zi]; else the LDS slot of this partial sum
};
struct DiagJoin {        // 16 bytes: W[zi] = slots slot, slot + 1, ... slot + count - 1 added in that order
  unsigned zi;
  int slot, count;
  int pad_;
};
struct DiagTable {
  std::vector<DiagTerm> terms;
  std::vector<DiagPiece> pieces;
  std::vector<DiagJoin> joins;
  int n_slots = 0;
};

// The checks of the five diagonal calls after the chunk's own, in this order: n_terms, null arguments, gamma (phase
// only: null otherwise), then term by term locality and a finite coefficient.  `per_term` is the caller's array of one
// double per term: the coefficients (`coeffs` true), or what qsim_expectation_z_terms writes to, which is never read.
static int check_diag_args(int k, int n_terms, const uint64_t* z_masks, const double* per_term, bool coeffs, const double* gamma,
                           const char* what) {
  if (n_terms < 0) return fail(QSIM_ERR_INVALID, "%s: n_terms = %d", what, n_terms);
  if (n_terms > kDiagMaxTerms) return fail(QSIM_ERR_INVALID, "%s: %d terms in one call, at most %d", what, n_terms, kDiagMaxTerms);
  if (n_terms > 0 && (!z_masks || !per_term)) return fail(QSIM_ERR_INVALID, "%s: null argument", what);
  if (gamma && !std::isfinite(*gamma)) return fail(QSIM_ERR_INVALID, "%s: gamma is not finite", what);
  const u64 all = k >= 64 ? ~0ull : (1ull << k) - 1;
  for (int t = 0; t < n_terms; ++t) {
    if (z_masks[t] & ~all)
      return fail(QSIM_ERR_NONLOCAL, "%s: term %d acts on index bit %d >= log2(chunk_size)=%d", what, t,
                  63 - __builtin_clzll(z_masks[t] & ~all), k);
    if (coeffs && !std::isfinite(per_term[t])) return fail(QSIM_ERR_INVALID, "%s: coefficient of term %d is not finite", what, t);
  }
  return QSIM_OK;
}

// the tables of a checked call on a chunk of k index bits with tiles of tb bits
static void diag_table(int tb, int n, const uint64_t* z_masks, const double* coeffs, DiagTable* d) {
  const u64 inner = (1ull << tb) - 1;
  std::vector<int> order((size_t)n);
  for (int t = 0; t < n; ++t) order[(size_t)t] = t;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return (z_masks[a] & inner) < (z_masks[b] & inner); });
  d->terms.resize((size_t)n);
  for (int i = 0; i < n; ++i) {
    const int t = order[(size_t)i];
    d->terms[(size_t)i].zo = z_masks[t] & ~inner;
    d->terms[(size_t)i].c = coeffs[t];
  }
  d->pieces.clear();
  d->joins.clear();
  d->n_slots = 0;
  for (int first = 0; first < n;) {
    const unsigned zi = (unsigned)(z_masks[order[(size_t)first]] & inner);
    int end = first + 1;
    while (end < n && (unsigned)(z_masks[order[(size_t)end]] & inner) == zi) ++end;
    const int len = end - first, n_pieces = (len + kDiagPiece - 1) / kDiagPiece;
    if (n_pieces > 1) {
      DiagJoin j = {zi, d->n_slots, n_pieces, 0};
      d->joins.push_back(j);
    }
    for (int p = 0; p < n_pieces; ++p) {
      DiagPiece pc = {first + p * kDiagPiece, std::min(kDiagPiece, len - p * kDiagPiece), zi, n_pieces > 1 ? d->n_slots++ : -1};
      d->pieces.push_back(pc);
    }
    first = end;
  }
}

// ---- the values of the single terms, <Z^{z_t}> = sum_i |psi_i|^2 (-1)^popcount(i & z_t) (qsim_expectation_z_terms,
// k_diag_term_values): the transpose of the table above.  With p_l = |psi_{base | l}|^2 over a tile,
//   sum_l p_l (-1)^popcount((base | l) & z) = (-1)^popcount(base & zo) WHT(p)[zi]:
// ONE transform of the tile's probabilities holds every Z string, a term is a gather at zi and the outer sign.  A pass
// over the state serves kDiagValuesPerPass terms, in INPUT order (nothing is sorted or merged: duplicates are served
// twice and get equal bits): pass p holds the terms p * kDiagValuesPerPass ..., and term i of a pass belongs to thread
// i % kBlock, register slot i / kBlock, for the whole launch.  The record carries no coefficient.
constexpr int kDiagValuesPerPass = 2048;
struct DiagValueTerm {   // 16 bytes, in input order
  u64 zo;                // z outside the tile (physical bits): the outer sign
  unsigned zi;           // z inside the tile: the index into the transformed probabilities
  unsigned pad_;
};
struct DiagValuePass {
  int first, count;      // terms first .. first + count - 1 of the list, 1 <= count <= kDiagValuesPerPass
};
struct DiagValueTable {
  std::vector<DiagValueTerm> terms;
  std::vector<DiagValuePass> passes;
};

// the records and the passes of a checked call on tiles of tb bits
static void diag_value_table(int tb, int n, const uint64_t* z_masks, DiagValueTable* d) {
  const u64 inner = (1ull << tb) - 1;
  d->terms.resize((size_t)n);
  for (int t = 0; t < n; ++t) {
    DiagValueTerm r = {z_masks[t] & ~inner, (unsigned)(z_masks[t] & inner), 0u};
    d->terms[(size_t)t] = r;
  }
  d->passes.clear();
  for (int first = 0; first < n; first += kDiagValuesPerPass) {
    DiagValuePass p = {first, std::min(kDiagValuesPerPass, n - first)};
    d->passes.push_back(p);
  }
}
