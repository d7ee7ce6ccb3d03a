// rdm_wide_plan.h -- host side of the reduced density matrix of 7 to 12 qubits (k_rdm_wide in rdm_kernels.h,
// qsim_reduced_density_matrix_wide in abi_readout.h): the argument checks, the role of every selected qubit, the tile,
// the work items and the way back from (block, row) coordinates to the caller's index.  Pure C++, no device call and
// no HIP type: tools/rdm_wide_plan_check.cpp compiles this file alone, with stubs for fail() and the error codes, under
// the host sanitizers.
// Part of the single translation unit qsim_hip.hip (included there before rdm_kernels.h; not a standalone header).
//
// rho is cut into 64 x 64 blocks.  Six of the r selected qubits are ROW qubits (bit rho of the position inside a
// block), the other r - 6 are BLOCK qubits (their pattern I < NB = 2^(r - 6) names the block).  Every selected qubit on
// a line bit (physical bit 0..2) is a row qubit, so a 128-byte line never holds amplitudes of two blocks; the rest of
// the six are the selected qubits on the lowest physical bits.  A tile is the line bits, the row qubits and the lowest
// non-selected bits up to kRdmWideTileBits (all there are in a small chunk); it is staged as 64 rows of E = 2^(tb - 6)
// words.  The outer index walks the bits that are neither tile bits nor block qubits.  A work item is a block pair
// (I, J), I >= J, times one of S slices of the outer index: slice s takes the outer tiles s, s + S, s + 2 S, ...
// Workgroup w = s * pairs + p writes its partial block (kRdmWideBlockDoubles doubles) at row s, column block p: the
// slices are rows for the row sum, added in slice order.
constexpr int kRdmWideMinQubits = 7;
constexpr int kRdmWideMaxQubits = 12;
constexpr int kRdmWideRowBits = 6;                   // 64 x 64 blocks
constexpr int kRdmWideTileBits = 11;                 // = kRdmTileBits (static_assert in rdm_kernels.h)
constexpr int kRdmWideLineBits = 3;                  // 8 amplitudes = one 128-byte line
constexpr int kRdmWideMaxWg = 2048;                  // pairs * S <= this (r = 12 has 2080 pairs: S = 1 there)
constexpr int kRdmWideBlockDoubles = 2 * 64 * 64;    // a partial block: Re [a * 64 + b], then Im at 4096 + the same

struct RdmWidePlan {
  int k, r;
  int tb, eb;                                        // tile bits; e' bits = tb - 6
  int nb_bits, nb;                                   // block qubits, NB = 2^nb_bits
  int row_phys[kRdmWideRowBits], row_pos[kRdmWideRowBits];   // row bit -> physical bit; -> its j with qubits[j] == that bit
  int blk_phys[kRdmWideMaxQubits - kRdmWideRowBits];         // block bit (ascending physical) -> physical bit
  int blk_pos[kRdmWideMaxQubits - kRdmWideRowBits];          // ... -> its j
  int phys_bit[kRdmWideTileBits], lds_pos[kRdmWideTileBits]; // as RdmArgs: tile bit (ascending physical) -> physical bit / LDS index bit
  u64 tile_mask, block_mask, outer_mask;             // disjoint, together all k bits
  u64 n_outer;                                       // 2^popcount(outer_mask)
  int pairs;                                         // NB (NB + 1) / 2, pair p = I (I + 1) / 2 + J (rdm_tile_row / _col)
  unsigned slices;                                   // S: a power of two <= n_outer, pairs * S <= max(max_wg, pairs)
  unsigned grid;                                     // pairs * S
  u64 work_bytes;                                    // the partial blocks and the summed ones
};

// The checks of the wide call after the chunk's own, in the order of check_qubit_list: null arguments, the range of r,
// (pending pieces: the caller's, between the two halves), then qubit by qubit range, locality and repetition.
static int rdm_wide_check_count(int r, const int32_t* qubits, const void* out, const char* what) {
  if (!qubits || !out) return fail(QSIM_ERR_INVALID, "%s: null argument", what);
  if (r < kRdmWideMinQubits || r > kRdmWideMaxQubits)
    return fail(QSIM_ERR_INVALID, "%s: %d <= r <= %d qubits expected, got %d (qsim_reduced_density_matrix serves r <= 6)", what,
                kRdmWideMinQubits, kRdmWideMaxQubits, r);
  return QSIM_OK;
}
static int rdm_wide_check_qubits(int k, int r, const int32_t* qubits, const char* what) {
  for (int i = 0; i < r; ++i) {
    const int q = qubits[i];
    if (q < 0) return fail(QSIM_ERR_INVALID, "qubit %d is negative", q);
    if (q >= k)
      return fail(QSIM_ERR_NONLOCAL, "qubit %d >= log2(chunk_size)=%d: non-local gate requires layout/collect step", q, k);
    for (int j = 0; j < i; ++j) if (qubits[j] == q) return fail(QSIM_ERR_INVALID, "%s: repeated qubit %d", what, q);
  }
  return QSIM_OK;
}

// The lower triangle row by row: t = I (I + 1) / 2 + J, I >= J.  The one definition for the 16 x 16 MFMA tiles of
// k_rdm_mfma, for the block pairs of k_rdm_wide and for the host (constexpr: usable on both sides).
constexpr int rdm_tile_row(int t) {                  // t -> I
  int i = 0;
  while ((i + 1) * (i + 2) / 2 <= t) ++i;
  return i;
}
constexpr int rdm_tile_col(int t) { return t - rdm_tile_row(t) * (rdm_tile_row(t) + 1) / 2; }

// the plan of a checked call (7 <= r <= 12 distinct qubits below k); max_wg: the cap on pairs * S (the host check lowers it)
static void rdm_wide_plan(int k, int r, const int32_t* qubits, RdmWidePlan* p, int max_wg = kRdmWideMaxWg) {
  std::memset(p, 0, sizeof *p);
  p->k = k;
  p->r = r;
  p->nb_bits = r - kRdmWideRowBits;
  p->nb = 1 << p->nb_bits;
  u64 sel = 0;
  for (int j = 0; j < r; ++j) sel |= 1ull << qubits[j];
  // roles: ascending physical order puts the line bits first, so the six lowest selected bits are the row qubits
  u64 rows = 0;
  int n_row = 0, n_blk = 0;
  for (int b = 0; b < k; ++b) {
    if (!((sel >> b) & 1)) continue;
    int j = 0;
    while (qubits[j] != b) ++j;
    if (n_row < kRdmWideRowBits) {
      p->row_phys[n_row] = b;
      p->row_pos[n_row++] = j;
      rows |= 1ull << b;
    } else {
      p->blk_phys[n_blk] = b;
      p->blk_pos[n_blk++] = j;
      p->block_mask |= 1ull << b;
    }
  }
  // the tile: line bits and row qubits, completed with the lowest non-selected bits
  p->tb = std::min(kRdmWideTileBits, k - p->nb_bits);
  p->eb = p->tb - kRdmWideRowBits;
  u64 T = rows | ((1ull << std::min(k, kRdmWideLineBits)) - 1);
  for (int b = 0; b < k && __builtin_popcountll(T) < p->tb; ++b)
    if (!((sel >> b) & 1)) T |= 1ull << b;
  p->tile_mask = T;
  int n_env = 0;
  for (int b = 0, t = 0; b < k; ++b) {
    if (!((T >> b) & 1)) continue;
    p->phys_bit[t] = b;
    if ((rows >> b) & 1) {
      for (int q = 0; q < kRdmWideRowBits; ++q) if (p->row_phys[q] == b) p->lds_pos[t] = p->eb + q;
    } else {
      p->lds_pos[t] = n_env++;
    }
    ++t;
  }
  const u64 all = (1ull << k) - 1;
  p->outer_mask = all & ~T & ~p->block_mask;
  p->n_outer = 1ull << (k - p->tb - p->nb_bits);
  p->pairs = p->nb * (p->nb + 1) / 2;
  unsigned s = 1;
  while ((u64)(2 * s) <= p->n_outer && (u64)p->pairs * (2 * s) <= (u64)max_wg) s *= 2;
  p->slices = s;
  p->grid = (unsigned)p->pairs * s;
  // rows of the row sum (S x pairs blocks), then the summed blocks (pairs); S = 1 needs no sum and no second part
  p->work_bytes = sizeof(double) * (u64)kRdmWideBlockDoubles * ((u64)p->grid + (s > 1 ? (u64)p->pairs : 0));
}

constexpr u64 rdm_wide_deposit(const int* blk_phys, int nb_bits, int I) {   // block pattern I on its physical bits (host and kernel)
  u64 d = 0;
  for (int b = 0; b < nb_bits; ++b) d |= (u64)((I >> b) & 1) << blk_phys[b];
  return d;
}
static u64 rdm_wide_deposit(const RdmWidePlan& p, int I) { return rdm_wide_deposit(p.blk_phys, p.nb_bits, I); }

static int rdm_wide_index(const RdmWidePlan& p, int I, int a) {   // (block I, row a) -> the caller's index (bit j <-> qubits[j])
  int x = 0;
  for (int q = 0; q < kRdmWideRowBits; ++q) x |= ((a >> q) & 1) << p.row_pos[q];
  for (int b = 0; b < p.nb_bits; ++b) x |= ((I >> b) & 1) << p.blk_pos[b];
  return x;
}

// The summed blocks [pair][kRdmWideBlockDoubles] -> out (2 * 4^r doubles, row-major complex).  Block (I, J), I > J, is
// written as it is and its conjugate transpose goes to (J, I); of a diagonal block only the triangle a >= b is read (the
// kernel computes no more) and mirrored, the imaginary diagonal is zero: out is exactly Hermitian.
static void rdm_wide_assemble(const RdmWidePlan& p, const double* blocks, double* out) {
  const u64 dim = 1ull << p.r;
  std::vector<int> idx((size_t)dim);
  for (int I = 0; I < p.nb; ++I)
    for (int a = 0; a < 64; ++a) idx[(size_t)(I * 64 + a)] = rdm_wide_index(p, I, a);
  for (int pr = 0; pr < p.pairs; ++pr) {
    const int I = rdm_tile_row(pr), J = rdm_tile_col(pr);
    const double* blk = blocks + (u64)pr * kRdmWideBlockDoubles;
    for (int a = 0; a < 64; ++a) {
      const u64 x = (u64)idx[(size_t)(I * 64 + a)];
      for (int b = 0; b < (I == J ? a + 1 : 64); ++b) {
        const u64 y = (u64)idx[(size_t)(J * 64 + b)];
        const double re = blk[a * 64 + b], im = (I == J && a == b) ? 0.0 : blk[4096 + a * 64 + b];
        out[2 * (x * dim + y)] = re;
        out[2 * (x * dim + y) + 1] = im;
        if (x != y) {
          out[2 * (y * dim + x)] = re;
          out[2 * (y * dim + x) + 1] = -im;
        }
      }
    }
  }
}
