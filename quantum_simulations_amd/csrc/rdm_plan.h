// rdm_plan.h -- host side of the reduced density matrices (rdm_kernels.h; qsim_reduced_density_matrix for r <= 6 and
// qsim_reduced_density_matrix_wide for r = 7..12 in abi_readout.h): the tile, the work items, the workspace and the way
// from what the device sums to the caller's matrix.  Pure C++, no device call and no HIP type:
// tools/rdm_plan_check.cpp compiles this file alone under the host sanitizers.
// Part of the single translation unit qsim_hip.hip (included there before rdm_kernels.h; not a standalone header).
//
// The tile (rdm_tile_layout), both calls.  Up to six selected qubits are ROW qubits: row bit q of the staged tile.  The
// tile bits are the line bits (physical bits 0..2: a 128-byte line is read whole), the row qubits and the lowest
// non-selected bits up to tb; the tile is staged as 2^rows rows of E = 2^eb words, LDS index = row * E + e'.  The outer
// index walks the bits that are neither tile bits nor selected.
//   r <= 6 (rdm_plan): every qubit is a row qubit, in the caller's order, so a row index is the caller's index.
//   Workgroup w takes the outer tiles w, w + grid, ...; it writes one partial matrix, the rows of the row sum.
//   r = 7..12 (rdm_wide_plan): rho is cut into 64 x 64 blocks.  The six selected qubits on the lowest physical bits are
//   the row qubits, in ascending order -- so every selected line bit is one and a line never holds amplitudes of two
//   blocks; the other r - 6 are BLOCK qubits, whose pattern I < NB = 2^(r - 6) names the block.  A work item is a block
//   pair (I, J), I >= J, times one of S slices of the outer index: slice s takes the outer tiles s, s + S, ...
//   Workgroup w = s * pairs + p writes its partial block at row s, column block p: the slices are the rows of the sum.
constexpr int kRdmTileBits = 11;                     // 2^11 amplitudes = 32 KiB of LDS, as the expectation pass
constexpr int kRdmRowBits = 6;                       // most row qubits: all of r <= 6, the 64 x 64 blocks beyond
constexpr int kRdmLineBits = 3;                      // 8 amplitudes = one 128-byte line
constexpr int kRdmMaxWg = 1024;                      // r <= 6, workgroups per launch: partial matrices <= 1024 * 4^r * 8 B
constexpr int kRdmWideMaxWg = 2048;                  // r >= 7: pairs * S <= this (r = 12 has 2080 pairs: S = 1 there)
constexpr int kRdmWideMinQubits = 7;
constexpr int kRdmWideMaxQubits = 12;
constexpr int kRdmWideBlockDoubles = 2 * 64 * 64;    // a partial block: Re [a * 64 + b], then Im at 4096 + the same

struct RdmTileLayout {
  int tb, eb;                                        // tile bits; e' bits = tb - rows
  int phys_bit[kRdmTileBits];                        // tile bit t in ascending physical order -> physical index bit
  int lds_pos[kRdmTileBits];                         // ... -> its bit of the LDS index: e' bits below (ascending), row bit q at eb + q
  u64 tile_mask, outer_mask;                         // disjoint; with the selected bits outside the tile, all k bits
  u64 n_tiles;                                       // 2^popcount(outer_mask)
};

// sel: every selected qubit; rows: the n_rows <= tb of them that are row qubits, in row order
static void rdm_tile_layout(int k, int tb, u64 sel, const int* rows, int n_rows, RdmTileLayout* t) {
  std::memset(t, 0, sizeof *t);
  t->tb = tb;
  t->eb = tb - n_rows;
  u64 T = (1ull << std::min(k, kRdmLineBits)) - 1;
  for (int q = 0; q < n_rows; ++q) T |= 1ull << rows[q];
  for (int b = 0; b < k && __builtin_popcountll(T) < tb; ++b)
    if (!((sel >> b) & 1)) T |= 1ull << b;
  t->tile_mask = T;
  int n_env = 0;
  for (int b = 0, j = 0; b < k; ++b) {
    if (!((T >> b) & 1)) continue;
    t->phys_bit[j] = b;
    t->lds_pos[j] = -1;
    for (int q = 0; q < n_rows; ++q) if (rows[q] == b) t->lds_pos[j] = t->eb + q;
    if (t->lds_pos[j] < 0) t->lds_pos[j] = n_env++;
    ++j;
  }
  t->outer_mask = ((1ull << k) - 1) & ~T & ~sel;
  t->n_tiles = 1ull << __builtin_popcountll(t->outer_mask);
}

// The lower triangle row by row: t = I (I + 1) / 2 + J, I >= J.  The one numbering of the 16 x 16 MFMA tiles of a
// matrix or block, of the 4 x 4 blocks of k_rdm_block and of the block pairs of k_rdm_wide (constexpr: host and kernel).
constexpr int rdm_tile_row(int t) {                  // t -> I
  int i = 0;
  while ((i + 1) * (i + 2) / 2 <= t) ++i;
  return i;
}
constexpr int rdm_tile_col(int t) { return t - rdm_tile_row(t) * (rdm_tile_row(t) + 1) / 2; }

// ---- r <= 6
struct RdmPlan {
  int r;
  RdmTileLayout t;
  int swz[kRdmRowBits];                              // r <= 3: row a is stored with e' ^ g(a), g(a) = XOR of swz[q] over the set bits q of a
  unsigned grid;                                     // min(n_tiles, max_wg)
  u64 work_bytes;                                    // grid partial matrices of 4^r doubles and the summed one
};

// the plan of a checked call (1 <= r <= 6 distinct qubits below k); max_wg: the cap on the grid (the host check lowers it)
static void rdm_plan(int k, int r, const int32_t* qubits, RdmPlan* p, int max_wg = kRdmMaxWg) {
  std::memset(p, 0, sizeof *p);
  p->r = r;
  u64 sel = 0;
  int rows[kRdmRowBits];
  for (int q = 0; q < r; ++q) { rows[q] = qubits[q]; sel |= 1ull << qubits[q]; }
  rdm_tile_layout(k, std::min(k, kRdmTileBits), sel, rows, r, &p->t);
  // The swizzle of k_rdm_small: the 8 lanes of a line differ in the row bits on line bits and would store to 8 rows at
  // one bank.  Each qubit on a line bit, in row order, therefore XORs the next of the e' bits 0..2 that the line bits
  // outside the qubits leave free (the e' bits below are those line bits, which the lanes of a line already differ in),
  // while there is such an e' bit.
  const int line = std::min(k, kRdmLineBits);
  int free_bit = line - __builtin_popcountll(sel & ((1ull << line) - 1));
  for (int q = 0; q < r; ++q)
    if (qubits[q] < kRdmLineBits && free_bit < std::min(p->t.eb, kRdmLineBits)) p->swz[q] = 1 << free_bit++;
  p->grid = (unsigned)std::min<u64>(p->t.n_tiles, (u64)max_wg);
  p->work_bytes = sizeof(double) * ((u64)p->grid + 1) << (2 * r);
}

// The summed triangle (D * D doubles, D = 2^r: Re rho[a][b], a >= b, at [a * D + b] and Im rho[a][b], a > b, at
// [b * D + a]) -> out (2 * 4^r doubles, row-major complex) with its mirror image: exactly Hermitian.
static void rdm_mirror(int r, const double* tri, double* out) {
  const int dim = 1 << r;
  for (int x = 0; x < dim; ++x) {
    out[2 * (x * dim + x)] = tri[x * dim + x];
    out[2 * (x * dim + x) + 1] = 0.0;
    for (int y = 0; y < x; ++y) {
      const double re = tri[x * dim + y], im = tri[y * dim + x];
      out[2 * (x * dim + y)] = re;
      out[2 * (x * dim + y) + 1] = im;
      out[2 * (y * dim + x)] = re;
      out[2 * (y * dim + x) + 1] = -im;
    }
  }
}

// ---- r = 7..12
struct RdmWidePlan {
  int k, r;
  RdmTileLayout t;                                   // six rows; its n_tiles are the outer tiles of one block pattern
  int nb_bits, nb;                                   // block qubits, NB = 2^nb_bits
  int row_phys[kRdmRowBits], row_pos[kRdmRowBits];   // row bit -> physical bit (ascending); -> its j with qubits[j] == that bit
  int blk_phys[kRdmWideMaxQubits - kRdmRowBits];     // block bit (ascending physical) -> physical bit
  int blk_pos[kRdmWideMaxQubits - kRdmRowBits];      // ... -> its j
  u64 block_mask;                                    // the block qubits: what tile_mask and outer_mask leave of the k bits
  int pairs;                                         // NB (NB + 1) / 2, pair p = I (I + 1) / 2 + J (rdm_tile_row / _col)
  unsigned slices;                                   // S: a power of two <= n_tiles, pairs * S <= max(max_wg, pairs)
  unsigned grid;                                     // pairs * S
  u64 work_bytes;                                    // the partial blocks and the summed ones
};

// the plan of a checked call (7 <= r <= 12 distinct qubits below k); max_wg: the cap on pairs * S (the host check lowers it)
static void rdm_wide_plan(int k, int r, const int32_t* qubits, RdmWidePlan* p, int max_wg = kRdmWideMaxWg) {
  std::memset(p, 0, sizeof *p);
  p->k = k;
  p->r = r;
  p->nb_bits = r - kRdmRowBits;
  p->nb = 1 << p->nb_bits;
  u64 sel = 0;
  for (int j = 0; j < r; ++j) sel |= 1ull << qubits[j];
  // roles: ascending physical order puts the line bits first, so the six lowest selected bits are the row qubits
  int n_row = 0, n_blk = 0;
  for (int b = 0; b < k; ++b) {
    if (!((sel >> b) & 1)) continue;
    int j = 0;
    while (qubits[j] != b) ++j;
    if (n_row < kRdmRowBits) {
      p->row_phys[n_row] = b;
      p->row_pos[n_row++] = j;
    } else {
      p->blk_phys[n_blk] = b;
      p->blk_pos[n_blk++] = j;
      p->block_mask |= 1ull << b;
    }
  }
  rdm_tile_layout(k, std::min(kRdmTileBits, k - p->nb_bits), sel, p->row_phys, kRdmRowBits, &p->t);
  p->pairs = p->nb * (p->nb + 1) / 2;
  unsigned s = 1;
  while ((u64)(2 * s) <= p->t.n_tiles && (u64)p->pairs * (2 * s) <= (u64)max_wg) s *= 2;
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
  for (int q = 0; q < kRdmRowBits; ++q) x |= ((a >> q) & 1) << p.row_pos[q];
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
