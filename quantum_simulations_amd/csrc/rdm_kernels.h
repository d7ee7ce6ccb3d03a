// rdm_kernels.h -- reduced density matrices: k_rdm_small (r = 1..3) and k_rdm_mfma (r = 4..6) for
// qsim_reduced_density_matrix, k_rdm_wide (r = 7..12 in 64 x 64 blocks) for qsim_reduced_density_matrix_wide; the host
// side of both is rdm_plan.h.
// Part of the single translation unit qsim_hip.hip (included there after rdm_plan.h; not a standalone header).
//
//   rho[a][b] = sum over e of psi(e, a) conj(psi(e, b)),   a, b < D = 2^r,  bit j of a <-> index bit qubits[j].
//
// One read-only pass, no atomics: two calls give the same bits.  The mechanisms, each written once:
//
// The tile walk (RdmTile, rdm_thread_slots, rdm_fetch, rdm_fill; every kernel).  A workgroup walks tiles of the layout
// of rdm_plan.h.  Global loads go in ascending physical order (8 consecutive lanes read one 128-byte line whatever the
// qubits are); the permutation is in the LDS address: LDS index = a * E + e', so psi(., a) is a contiguous row and the
// sums need no bit gathering.  The next tile's 8 loads per thread are requested right after the current tile is in LDS,
// so they are in flight under the sums.  Accumulators stay in registers across all tiles of a workgroup, which writes
// one partial result at the end; k_hist_sum adds the partial results in workgroup (or slice) order.
//
// The partial matrix of r <= 6 (rdm_tri_index).  Only the lower triangle is computed: D * D doubles, Re rho[a][b], a >= b,
// at [a * D + b] and Im rho[a][b], a > b, at [b * D + a]; the host mirrors it (rdm_mirror).
//
// k_rdm_small: a thread per e' (consecutive lanes read consecutive 16-byte words of a row: no bank conflicts) that holds
// the whole triangle.  Line bits among the qubits would make the 8 lanes of a line store to 8 rows at the same bank; row
// a is therefore stored with e' ^ g(a) (swz[] of rdm_plan; a thread reads row a with the same XOR: a permutation inside
// aligned groups of 8 words).  At the end each accumulator is folded over the wave (butterfly) and the four waves are
// added in wave order.
//
// The matrix cores (k_rdm_mfma, k_rdm_wide): v_mfma_f64_16x16x4_f64 on the real image.  With X[a][k] = component k & 1
// of psi(e' = k >> 1, a) and X'[a][k] = (Im, -Re) in place of (Re, Im):  Re rho = X X^T,  Im rho = X' X^T.  rho, or a
// block of it, is cut into 16 x 16 tiles (I, J), numbered by rdm_tile_row / rdm_tile_col; a UNIT u = 2 * tile + (Re, Im)
// is 4 accumulator doubles per lane.  Operand layouts as in dense_kernels.h (lane l: j = l & 15, g = l >> 4):
// A[row j][k g], B[k g][column j], D element i = [row 4 i + g][column j] -- so the A operand of row block I and the B
// operand of column block I are the same register: a lane reads ONE 16-byte word per row block and k-step of two e',
// psi(2 s + (g >> 1), 16 I + j), and picks (p, q) = its component of X and X' from it (rdm_pick; a zero operand where
// the chunk has no second e').  Rows are padded by one word (row stride E + 1): the 16 lanes of an LDS group read 16
// rows at the same e', 16 different words of a bank span, and the 8 lanes of a line store to 8 rows at 8 different banks
// whatever the qubits are.
//   r = 4, 5 (1, 3 tiles with I >= J = 2, 6 units): a wave keeps every unit and takes every fourth k-step; the four
//   waves' accumulators are added in wave order at the end.
//   64 rows on the diagonal (rdm_diag_step; r = 6 and the diagonal pairs of k_rdm_wide): 10 tiles = 20 units.  80
//   accumulator doubles per lane would leave one workgroup per CU, so wave W owns the units W, W + 4, .. -- five, by a
//   dispatch on the wave that keeps the unit indices compile-time constants (rdm_for_wave) -- over every k-step and
//   stores them itself (rdm_store_own_units, with the caller's destination index).
//   k_rdm_wide: six ROW qubits inside a block, r - 6 BLOCK qubits whose pattern names it.  Workgroup w = s * pairs + p
//   takes the block pair p = (I, J), I >= J, and slice s of the outer tiles: per outer tile it stages the tile of pattern
//   I (the pattern deposited on the block qubits' physical bits) and, off the diagonal, the one of pattern J in a
//   second LDS region.  Off the diagonal Re = X_I X_J^T, Im = X'_I X_J^T is 16 tiles = 32 units: wave W owns row block W
//   of I against the four column blocks of J, 8 units, one LDS word of I and four of J per k-step.  The workgroup writes
//   its partial block (Re [a * 64 + b], Im at 4096 + the same; of a diagonal block only the tiles of the lower triangle).
//
// k_rdm_block (probe build, QSIM_RDM_FORM=1: the first form of r = 4..6, fp64 vector FMAs, measured next to the matrix
// cores in profiles/r13_rdm_probe_vector_fma.json): a thread owns a 4 x 4 block (I, J), I >= J, of the D/4 x D/4 grid of
// blocks -- 10, 36, 136 blocks -- and one of 16, 4, 1 slices of e': 4 + 4 LDS reads for 16 complex multiply-adds per e'.
// Lanes of one 16-lane LDS group read different words of a 256-byte bank span: the slice, and for fewer than 16 slices a
// rotation of the walk over e' by the block number.  The slices of a block are added in slice order.  136 of 256 lanes
// work at r = 6 and a wave's instruction costs the same with 8 lanes as with 64, which is what the matrix cores do not pay.
static_assert(kRdmLineBits == kExpLineBits, "a line of the expectation pass");
constexpr int kRdmTile = 1 << kRdmTileBits;
constexpr int kRdmLoads = kRdmTile / kBlock;
constexpr int kRdmWaves = kBlock / 64;

struct RdmTile {                   // what the tile walk reads
  const double2* amp;
  u64 n_tiles;                     // outer tiles
  u64 outer_mask;                  // outer index bit j <-> the j-th set bit
  int phys_bit[kRdmTileBits];      // as RdmTileLayout
  int lds_pos[kRdmTileBits];
  int tb;
};
struct RdmArgs : RdmTile {
  double* partial;                 // [workgroup][4^r]
  int swz[kRdmRowBits];
};
struct RdmWideArgs : RdmTile {
  double* partial;                 // [slice][pair][kRdmWideBlockDoubles]
  int blk_phys[kRdmWideMaxQubits - kRdmRowBits];   // block bit -> physical bit
  int nb_bits;
  int pairs;
  unsigned slices;
};

static void rdm_tile_args(const RdmTileLayout& t, const qsim_chunk* c, RdmTile* a) {
  a->amp = c->amp;
  a->n_tiles = t.n_tiles;
  a->outer_mask = t.outer_mask;
  a->tb = t.tb;
  for (int b = 0; b < t.tb; ++b) { a->phys_bit[b] = t.phys_bit[b]; a->lds_pos[b] = t.lds_pos[b]; }
}

// physical offset and LDS index of the amplitudes this thread loads in every tile (swz: rows stored with e' ^ g(a))
template <int R, bool PAD>
__device__ __forceinline__ void rdm_thread_slots(const RdmTile& a, const int* swz, u64* off, int* lidx) {
  const int eb = a.tb - R;
#pragma unroll
  for (int it = 0; it < kRdmLoads; ++it) {
    const int j = (int)threadIdx.x + it * kBlock;
    u64 o = 0;
    int l = 0;
    for (int b = 0; b < a.tb; ++b) {
      o |= (u64)((j >> b) & 1) << a.phys_bit[b];
      l |= ((j >> b) & 1) << a.lds_pos[b];
    }
    if (swz) {
      int g = 0;
#pragma unroll
      for (int q = 0; q < R; ++q) g ^= ((l >> (eb + q)) & 1) ? swz[q] : 0;
      l ^= g;
    }
    if (PAD) l += l >> eb;                          // row stride E + 1
    off[it] = o;
    lidx[it] = l;
  }
}

template <bool NT>
__device__ __forceinline__ void rdm_fetch(const RdmTile& a, u64 o, const u64* off, double2* x) {   // tile o -> registers
  if (o >= a.n_tiles) return;
  const int S = 1 << a.tb;
  const u64 base = tile_base(a.outer_mask, o);       // pauli_tile.h
#pragma unroll
  for (int it = 0; it < kRdmLoads; ++it)
    if ((int)threadIdx.x + it * kBlock < S) x[it] = ld_amp<NT>(a.amp + (base | off[it]));
}

// registers -> the staged tile (chunks of fewer amplitudes than a tile: the threads that hold one)
__device__ __forceinline__ void rdm_fill(const RdmTile& a, double2* tile, const int* lidx, const double2* x) {
  const int S = 1 << a.tb;
#pragma unroll
  for (int it = 0; it < kRdmLoads; ++it)
    if ((int)threadIdx.x + it * kBlock < S) tile[lidx[it]] = x[it];
}
__device__ __forceinline__ void rdm_stage(const RdmTile& a, double2* tile, const int* lidx, const double2* x) {
  __syncthreads();                                  // (the previous tile is consumed)
  rdm_fill(a, tile, lidx, x);
  __syncthreads();
}

template <int D>
__device__ __forceinline__ int rdm_tri_index(int im, int x, int y) {   // where a partial matrix keeps Re / Im rho[x][y]; < 0: nowhere
  return im ? (x > y ? y * D + x : -1) : (x >= y ? x * D + y : -1);
}

template <int R, bool NT>
__global__ __launch_bounds__(kBlock) void k_rdm_small(const RdmArgs a) {
  static_assert(R >= 1 && R <= 3, "the whole triangle in one thread's registers");
  constexpr int D = 1 << R;
  __shared__ double2 tile[kRdmTile];
  const int tid = threadIdx.x;
  const int eb = a.tb - R, E = 1 << eb;
  u64 off[kRdmLoads];
  int lidx[kRdmLoads];
  rdm_thread_slots<R, false>(a, a.swz, off, lidx);
  int g[D];
#pragma unroll
  for (int x = 0; x < D; ++x) {
    g[x] = 0;
#pragma unroll
    for (int q = 0; q < R; ++q) g[x] ^= ((x >> q) & 1) ? a.swz[q] : 0;
  }
  double acc[D * D];                                // the layout of a partial matrix
#pragma unroll
  for (int s = 0; s < D * D; ++s) acc[s] = 0.0;
  double2 nxt[kRdmLoads];                           // the tile on its way
  rdm_fetch<NT>(a, blockIdx.x, off, nxt);
  for (u64 o = blockIdx.x; o < a.n_tiles; o += gridDim.x) {
    rdm_stage(a, tile, lidx, nxt);
    rdm_fetch<NT>(a, o + gridDim.x, off, nxt);
    for (int e = tid; e < E; e += kBlock) {
      double2 v[D];
#pragma unroll
      for (int x = 0; x < D; ++x) v[x] = tile[(x << eb) | (e ^ g[x])];
#pragma unroll
      for (int x = 0; x < D; ++x) {
        acc[x * D + x] = fma(v[x].x, v[x].x, fma(v[x].y, v[x].y, acc[x * D + x]));
#pragma unroll
        for (int y = 0; y < x; ++y) {
          acc[x * D + y] = fma(v[x].x, v[y].x, fma(v[x].y, v[y].y, acc[x * D + y]));
          acc[y * D + x] = fma(v[x].y, v[y].x, fma(-v[x].x, v[y].y, acc[y * D + x]));
        }
      }
    }
  }
  __syncthreads();
  double* red = reinterpret_cast<double*>(tile);    // [wave][D * D]
#pragma unroll
  for (int s = 0; s < D * D; ++s) {
    const double v = wave_sum(acc[s]);
    if ((tid & 63) == 0) red[(tid >> 6) * D * D + s] = v;
  }
  __syncthreads();
  for (int s = tid; s < D * D; s += kBlock) {
    double v = red[s];
    for (int w = 1; w < kBlock / 64; ++w) v += red[w * D * D + s];
    a.partial[(u64)blockIdx.x * (D * D) + s] = v;
  }
}

#ifdef QSIM_PROBES         // (the vector-ALU form of r = 4..6: the A/B partner of k_rdm_mfma below)
template <int R, bool NT>
__global__ __launch_bounds__(kBlock) void k_rdm_block(const RdmArgs a) {
  static_assert(R >= 4 && R <= kRdmRowBits, "4 x 4 blocks");
  constexpr int D = 1 << R, DB = D / 4, NB = DB * (DB + 1) / 2;
  constexpr int SL = R == 4 ? 16 : R == 5 ? 4 : 1;  // slices of e' per block: 160, 144, 136 threads at work
  static_assert(NB * SL <= kBlock, "a thread per (block, slice)");
  __shared__ double2 tile[kRdmTile];
  const int tid = threadIdx.x;
  const int eb = a.tb - R, E = 1 << eb;
  u64 off[kRdmLoads];
  int lidx[kRdmLoads];
  rdm_thread_slots<R, false>(a, nullptr, off, lidx);
  const int blk = tid / SL, slice = tid % SL;
  const int sl = SL < E ? SL : E;                   // slices at work (small chunks: fewer e' than slices)
  const int L = E / sl;                             // e' per slice: slice + sl * 0 .. slice + sl * (L - 1)
  const bool active = blk < NB && slice < sl;
  const int I = active ? rdm_tile_row(blk) : 0, J = active ? rdm_tile_col(blk) : 0;
  const int rot = SL < 16 ? (blk & (16 / SL - 1)) : 0;
  const double2* row_a = tile + ((4 * I) << eb) + slice;
  const double2* row_b = tile + ((4 * J) << eb) + slice;
  double re[16], im[16];
#pragma unroll
  for (int v = 0; v < 16; ++v) re[v] = im[v] = 0.0;
  double2 nxt[kRdmLoads];                           // the tile on its way
  rdm_fetch<NT>(a, blockIdx.x, off, nxt);
  for (u64 o = blockIdx.x; o < a.n_tiles; o += gridDim.x) {
    rdm_stage(a, tile, lidx, nxt);
    rdm_fetch<NT>(a, o + gridDim.x, off, nxt);
    if (!active) continue;
    for (int s = 0; s < L; ++s) {
      const int e = sl * ((s + rot) & (L - 1));
      double2 u[4], w[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        u[i] = row_a[(i << eb) + e];
        w[i] = row_b[(i << eb) + e];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          re[i * 4 + j] = fma(u[i].x, w[j].x, fma(u[i].y, w[j].y, re[i * 4 + j]));
          im[i * 4 + j] = fma(u[i].y, w[j].x, fma(-u[i].x, w[j].y, im[i * 4 + j]));
        }
    }
  }
  double* red = reinterpret_cast<double*>(tile);    // [entry of the block][thread]: 16 * kBlock doubles = the tile
  double* mine = a.partial + (u64)blockIdx.x * (D * D);
#pragma unroll
  for (int part = 0; part < 2; ++part) {            // the real parts, then the imaginary parts
    __syncthreads();
#pragma unroll
    for (int v = 0; v < 16; ++v) red[v * kBlock + tid] = part ? im[v] : re[v];
    __syncthreads();
    for (int t = tid; t < NB * 16; t += kBlock) {
      const int b = t >> 4, v = t & 15;
      const double* r = red + v * kBlock + b * SL;
      double sum = r[0];
      for (int q = 1; q < SL; ++q) sum += r[q];
      const int d = rdm_tri_index<D>(part, 4 * rdm_tile_row(b) + (v >> 2), 4 * rdm_tile_col(b) + (v & 3));
      if (d >= 0) mine[d] = sum;
    }
  }
}
#endif  // QSIM_PROBES

// (p, q) = the lane's component of X and X' from its word v; a zero operand unless `use`.  v is passed by value: the
// LDS read stays unconditional (the word exists whatever `use` is) and the choice is two selects, so the reads of a
// k-step are issued together instead of one branch and one wait each.
__device__ __forceinline__ void rdm_pick(const double2 v, bool im, bool use, double* p, double* q) {
  *p = use ? (im ? v.y : v.x) : 0.0;
  *q = use ? (im ? -v.x : v.y) : 0.0;
}

// f(std::integral_constant<int, wave>): the wave as a compile-time constant, so that what f indexes by it stays in registers
template <class F>
__device__ __forceinline__ void rdm_for_wave(int wave, F f) {
  static_assert(kRdmWaves == 4, "a case per wave");
  switch (wave) {
    case 0: f(std::integral_constant<int, 0>()); break;
    case 1: f(std::integral_constant<int, 1>()); break;
    case 2: f(std::integral_constant<int, 2>()); break;
    default: f(std::integral_constant<int, 3>()); break;
  }
}

// One k-step of the 20 units of 64 rows on the diagonal: the lane's words of the four row blocks at k-step s (row: its
// word of row block 0 at k-step 0, stride: E + 1), then the wave's five units.
__device__ __forceinline__ void rdm_diag_step(const double2* row, int stride, int s, bool im, bool use, int wave, qs_double4_t* acc) {
  double p[4], q[4];
#pragma unroll
  for (int b = 0; b < 4; ++b) rdm_pick(row[(16 * b) * stride + 2 * s], im, use, &p[b], &q[b]);
  rdm_for_wave(wave, [&](auto W) {
#pragma unroll
    for (int c = 0; c < 5; ++c) {
      const int u = decltype(W)::value + kRdmWaves * c, I = rdm_tile_row(u >> 1), J = rdm_tile_col(u >> 1);
      acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64((u & 1) ? q[I] : p[I], p[J], acc[c], 0, 0, 0);
    }
  });
}
// ... and their way out: index(Re / Im, row, column) is where the element goes in `mine`, < 0 for nowhere
template <class Index>
__device__ __forceinline__ void rdm_store_own_units(const qs_double4_t* acc, double* mine, int wave, int j, int g, Index index) {
  rdm_for_wave(wave, [&](auto W) {
#pragma unroll
    for (int c = 0; c < 5; ++c) {
      const int u = decltype(W)::value + kRdmWaves * c, I = rdm_tile_row(u >> 1), J = rdm_tile_col(u >> 1);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int d = index(u & 1, 16 * I + 4 * i + g, 16 * J + j);
        if (d >= 0) mine[d] = acc[c][i];
      }
    }
  });
}

template <int R, bool NT>
__global__ __launch_bounds__(kBlock) void k_rdm_mfma(const RdmArgs a) {
  static_assert(R >= 4 && R <= kRdmRowBits, "16 x 16 tiles");
  constexpr int D = 1 << R, NB = D / 16, NTILE = NB * (NB + 1) / 2, NU = 2 * NTILE;   // units: (tile, Re / Im)
  constexpr bool kOwnUnits = R == 6;                // all k-steps and a quarter of the units, not the reverse
  __shared__ double2 tile[kRdmTile + D];            // D rows of E + 1 words; later the waves' accumulators
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 15, g = lane >> 4;
  const int eb = a.tb - R, E = 1 << eb;
  u64 off[kRdmLoads];
  int lidx[kRdmLoads];
  rdm_thread_slots<R, true>(a, nullptr, off, lidx);
  const int steps = E > 1 ? E >> 1 : 1;             // k-steps of two e' (E = 1: the second e' is a zero operand)
  const bool real_e = (g >> 1) < E;
  const bool im = g & 1;
  const double2* row = tile + j * (E + 1) + (real_e ? g >> 1 : 0);
  constexpr int NACC = kOwnUnits ? 5 : NU;
  constexpr int kAhead = NB == 1 ? 4 : 1;           // r = 4: one LDS read feeds two MFMAs only, so four k-steps at a time
  qs_double4_t acc[NACC];
#pragma unroll
  for (int u = 0; u < NACC; ++u) acc[u] = qs_double4_t{0.0, 0.0, 0.0, 0.0};
  double2 nxt[kRdmLoads];                           // the tile on its way
  rdm_fetch<NT>(a, blockIdx.x, off, nxt);
  for (u64 o = blockIdx.x; o < a.n_tiles; o += gridDim.x) {
    rdm_stage(a, tile, lidx, nxt);
    rdm_fetch<NT>(a, o + gridDim.x, off, nxt);
    if constexpr (kOwnUnits) {
      for (int s = 0; s < steps; ++s) rdm_diag_step(row, E + 1, s, im, real_e, wave, acc);
    } else {
      // kAhead k-steps at a time: their LDS reads are in flight before the first MFMA waits for one (r = 4: 4.85 -> 3.95 ms
      // at 30 qubits; r = 5 with two at a time drops to 3 waves per SIMD and gains nothing).  Steps beyond the last one,
      // in chunks of fewer amplitudes than a tile, are zero operands.
      for (int s0 = wave; s0 < steps; s0 += kAhead * kRdmWaves) {
        double p[kAhead][NB], q[kAhead][NB];        // X and X' of the lane's row of every row block
#pragma unroll
        for (int n = 0; n < kAhead; ++n) {
          const int s = s0 + n * kRdmWaves;
#pragma unroll
          for (int b = 0; b < NB; ++b)
            rdm_pick(row[(16 * b) * (E + 1) + 2 * (s < steps ? s : s0)], im, real_e && s < steps, &p[n][b], &q[n][b]);
        }
#pragma unroll
        for (int n = 0; n < kAhead; ++n)
#pragma unroll
          for (int t = 0; t < NTILE; ++t) {
            acc[2 * t] = __builtin_amdgcn_mfma_f64_16x16x4f64(p[n][rdm_tile_row(t)], p[n][rdm_tile_col(t)], acc[2 * t], 0, 0, 0);
            acc[2 * t + 1] = __builtin_amdgcn_mfma_f64_16x16x4f64(q[n][rdm_tile_row(t)], p[n][rdm_tile_col(t)], acc[2 * t + 1], 0, 0, 0);
          }
      }
    }
  }
  double* mine = a.partial + (u64)blockIdx.x * (D * D);
  if constexpr (kOwnUnits) {                        // a unit lives in one wave: straight from the accumulators
    rdm_store_own_units(acc, mine, wave, j, g, [](int part, int x, int y) { return rdm_tri_index<D>(part, x, y); });
    return;
  }
  // the waves' accumulators in wave order, four units per round: red[unit of the round][wave][element i][lane]
  double* red = reinterpret_cast<double*>(tile);
  constexpr int kPerRound = 4;
  static_assert(kPerRound * kRdmWaves * kBlock <= 2 * kRdmTile, "a round fits the tile");
#pragma unroll
  for (int u0 = 0; u0 < NU; u0 += kPerRound) {
    __syncthreads();
#pragma unroll
    for (int c = 0; c < kPerRound; ++c)
      if (u0 + c < NACC) {
#pragma unroll
        for (int i = 0; i < 4; ++i) red[((c * kRdmWaves + wave) * 4 + i) * 64 + lane] = acc[u0 + c][i];
      }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < kPerRound; ++c)
      if (u0 + c < NU) {
        const int u = u0 + c;
        double sum = red[(c * kRdmWaves) * kBlock + tid];           // thread tid = element tid >> 6 of lane tid & 63
        for (int w = 1; w < kRdmWaves; ++w) sum += red[(c * kRdmWaves + w) * kBlock + tid];
        const int d = rdm_tri_index<D>(u & 1, 16 * rdm_tile_row(u >> 1) + 4 * wave + g, 16 * rdm_tile_col(u >> 1) + j);
        if (d >= 0) mine[d] = sum;
      }
  }
}

constexpr int kRdmWideRegion = 64 * ((kRdmTile >> 6) + 1);   // words of one staged tile: 64 rows of E + 1

template <bool NT>
__global__ __launch_bounds__(kBlock) void k_rdm_wide(const RdmWideArgs a) {
  __shared__ double2 tile[2 * kRdmWideRegion];
  double2* const tile_i = tile;
  double2* const tile_j = tile + kRdmWideRegion;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 15, g = lane >> 4;
  const int eb = a.tb - 6, E = 1 << eb;
  const int pair = (int)(blockIdx.x % (unsigned)a.pairs);
  const u64 slice = blockIdx.x / (unsigned)a.pairs;
  const int I = rdm_tile_row(pair), J = rdm_tile_col(pair);
  const bool diag = I == J;
  RdmTile ai = a, aj = a;          // the two patterns' tiles: the deposit is disjoint from every other bit of an offset
  ai.amp += rdm_wide_deposit(a.blk_phys, a.nb_bits, I);
  aj.amp += rdm_wide_deposit(a.blk_phys, a.nb_bits, J);
  u64 off[kRdmLoads];
  int lidx[kRdmLoads];
  rdm_thread_slots<6, true>(a, nullptr, off, lidx);
  const int steps = E > 1 ? E >> 1 : 1;             // k-steps of two e' (E = 1: the second e' is a zero operand)
  const bool real_e = (g >> 1) < E;
  const bool im = g & 1;
  const int row_off = j * (E + 1) + (real_e ? g >> 1 : 0);
  qs_double4_t acc[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) acc[u] = qs_double4_t{0.0, 0.0, 0.0, 0.0};
  double2 nxt_i[kRdmLoads], nxt_j[kRdmLoads];       // the tiles on their way
  rdm_fetch<NT>(ai, slice, off, nxt_i);
  if (!diag) rdm_fetch<NT>(aj, slice, off, nxt_j);
  for (u64 o = slice; o < a.n_tiles; o += a.slices) {
    __syncthreads();                                // (the previous tiles are consumed)
    rdm_fill(a, tile_i, lidx, nxt_i);
    if (!diag) rdm_fill(a, tile_j, lidx, nxt_j);
    __syncthreads();
    rdm_fetch<NT>(ai, o + a.slices, off, nxt_i);
    if (!diag) rdm_fetch<NT>(aj, o + a.slices, off, nxt_j);
    if (diag) {
      for (int s = 0; s < steps; ++s) rdm_diag_step(tile_i + row_off, E + 1, s, im, real_e, wave, acc);
    } else {
      const double2* row_i = tile_i + row_off + (16 * wave) * (E + 1);
      const double2* row_j = tile_j + row_off;
      for (int s = 0; s < steps; ++s) {
        double pi, qi, pj[4], unused;
        rdm_pick(row_i[2 * s], im, real_e, &pi, &qi);
#pragma unroll
        for (int b = 0; b < 4; ++b) rdm_pick(row_j[(16 * b) * (E + 1) + 2 * s], im, real_e, &pj[b], &unused);
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          acc[2 * b] = __builtin_amdgcn_mfma_f64_16x16x4f64(pi, pj[b], acc[2 * b], 0, 0, 0);
          acc[2 * b + 1] = __builtin_amdgcn_mfma_f64_16x16x4f64(qi, pj[b], acc[2 * b + 1], 0, 0, 0);
        }
      }
    }
  }
  double* mine = a.partial + (slice * (u64)a.pairs + (u64)pair) * kRdmWideBlockDoubles;
  if (diag) {
    rdm_store_own_units(acc, mine, wave, j, g, [](int part, int x, int y) { return part * 4096 + x * 64 + y; });
  } else {
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        mine[(16 * wave + 4 * i + g) * 64 + 16 * b + j] = acc[2 * b][i];
        mine[4096 + (16 * wave + 4 * i + g) * 64 + 16 * b + j] = acc[2 * b + 1][i];
      }
  }
}
