// rdm_kernels.h -- reduced density matrix of r <= 6 qubits (qsim_reduced_density_matrix) and, at the end of the file,
// of 7 to 12 qubits in 64 x 64 blocks (k_rdm_wide, qsim_reduced_density_matrix_wide).
// Part of the single translation unit qsim_hip.hip (included there after expect_kernels.h; not a standalone header).
//
//   rho[a][b] = sum over e of psi(e, a) conj(psi(e, b)),   a, b < D = 2^r,  bit j of a <-> index bit qubits[j].
//
// One read-only pass in the form of k_expect_tile.  The tile bits are the line bits 0..2 and the r qubits (at most 9
// forced bits), completed with the lowest free bits to min(k, 11): one pass always suffices.  A workgroup walks tiles
// with a grid-stride loop.  Global loads go in ascending physical order (8 consecutive lanes read one 128-byte line
// whatever the qubits are); the permutation is in the LDS address: LDS index = a * E + e', E = 2^(tb - r), so psi(., a)
// is a contiguous row and the sums need no bit gathering.  Every thread keeps its accumulators in registers across all
// its tiles and the workgroup writes one partial matrix at the end; k_hist_sum adds the partial matrices in workgroup
// order.  No atomics: two calls give the same bits.  Only the lower triangle is computed (a >= b); a partial matrix is
// D * D doubles: Re rho[a][b] at [a * D + b] and, for a > b, Im rho[a][b] at [b * D + a]; the host mirrors it.
//
// r = 1..3 (k_rdm_small): a thread per e' (consecutive lanes read consecutive 16-byte words of a row: no bank
// conflicts) that holds the whole triangle, D * D doubles.  Line bits among the qubits would make the 8 lanes of a line
// store to 8 rows at the same bank; the row is therefore stored with e' ^ g(a), g built from e' bits 0..2 that no line
// bit occupies (a thread reads row a with the same XOR: a permutation inside aligned groups of 8 words).  At the end
// each accumulator is folded over the wave (butterfly) and the four waves are added in wave order.
//
// r = 4..6 (k_rdm_mfma): the matrix cores, v_mfma_f64_16x16x4_f64 on the real image.  With X[a][k] = component k & 1
// of psi(e' = k >> 1, a) and X'[a][k] = (Im, -Re) in place of (Re, Im):  Re rho = X X^T,  Im rho = X' X^T.  rho is cut
// into 16 x 16 tiles (I, J); 1, 3, 10 tiles with I >= J of both products = 2, 6, 20 units of 4 accumulator doubles per
// lane.  r = 4, 5: a wave keeps every unit and takes every fourth k-step of 4 (two e'); the four waves' accumulators
// are added in wave order at the end.  r = 6: 80 accumulator doubles per lane would leave one workgroup per CU, so a
// wave owns 5 of the 20 units over every k-step and stores them itself.  Operand layouts as in dense_kernels.h (lane l:
// j = l & 15, g = l >> 4): A[row j][k g], B[k g][column j], D element i = [row 4 i + g][column j] -- so the A operand of
// row block I and the B operand of column block I are the same register: a lane reads ONE 16-byte word per row block
// and k-step, psi(2 s + (g >> 1), 16 I + j), for 2 (NB + 1) NB / 2 MFMAs.  Rows are padded by one word (row stride E + 1):
// the 16 lanes of an LDS group read 16 rows at the same e', 16 different words of a bank span, and the 8 lanes of a
// line store to 8 rows at 8 different banks whatever the qubits are.  The first form of this kernel, fp64 vector FMAs
// on 4 x 4 blocks per thread (k_rdm_block, kept in the probe build: QSIM_RDM_FORM=1), is measured next to it in
// profiles/r13_rdm_probe_vector_fma.json.
//
// k_rdm_block: a thread owns a 4 x 4 block (I, J), I >= J, of the D/4 x D/4 grid of blocks -- 10, 36, 136 blocks -- and
// one of 16, 4, 1 slices of e': 4 + 4 LDS reads for 16 complex multiply-adds per e'.  Lanes of one 16-lane LDS group read
// different words of a 256-byte bank span: the slice, and for fewer than 16 slices a rotation of the walk over e' by the
// block number.  The slices of a block are added in slice order.  136 of 256 lanes work at r = 6 and a wave's
// instruction costs the same with 8 lanes as with 64, which is what the matrix cores do not pay.
//
// Every kernel requests the next tile's 8 loads per thread right after the current tile is in LDS, so they are in flight
// under the sums.
constexpr int kRdmTileBits = 11;                    // 2^11 amplitudes = 32 KiB of LDS, as the expectation pass
constexpr int kRdmMaxWg = 1024;                     // workgroups per launch, every r: partial matrices <= 1024 * 4^r * 8 B
constexpr int kRdmMaxQubits = 6;

struct RdmArgs {
  const double2* amp;
  double* partial;                 // [workgroup][4^r]
  u64 n_tiles;                     // 2^(k - tb)
  u64 outer_mask;                  // physical bits outside the tile (outer index bit j <-> the j-th set bit)
  int phys_bit[kRdmTileBits];      // tile bit b in ascending physical order -> physical index bit
  int lds_pos[kRdmTileBits];       // ... -> its bit of the LDS index (e' bits below, then a bit j <-> qubits[j])
  int swz[kRdmMaxQubits];          // r <= 3: g(a) = XOR over the set bits j of a of swz[j] (0 unless qubits[j] < 3)
  int tb;                          // tile bits, >= r
};

constexpr int kRdmTile = 1 << kRdmTileBits;
constexpr int kRdmLoads = kRdmTile / kBlock;

// physical offset and LDS index of the amplitudes this thread loads in every tile (SWZ: rows stored with e' ^ g(a))
template <int R, bool SWZ, bool PAD = false>
__device__ __forceinline__ void rdm_thread_slots(const RdmArgs& a, u64* off, int* lidx) {
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
    if (SWZ) {
      int g = 0;
#pragma unroll
      for (int q = 0; q < R; ++q) g ^= ((l >> (eb + q)) & 1) ? a.swz[q] : 0;
      l ^= g;
    }
    if (PAD) l += l >> eb;                          // row stride E + 1
    off[it] = o;
    lidx[it] = l;
  }
}

template <bool NT>
__device__ __forceinline__ void rdm_fetch(const RdmArgs& a, u64 o, const u64* off, double2* x) {   // tile o -> registers
  if (o >= a.n_tiles) return;
  const int S = 1 << a.tb;
  const u64 base = tile_base(a.outer_mask, o);       // pauli_tile.h
#pragma unroll
  for (int it = 0; it < kRdmLoads; ++it)
    if ((int)threadIdx.x + it * kBlock < S) x[it] = ld_amp<NT>(a.amp + (base | off[it]));
}

__device__ __forceinline__ void rdm_stage(const RdmArgs& a, double2* tile, const int* lidx, const double2* x) {
  const int S = 1 << a.tb;
  __syncthreads();                                  // (the previous tile is consumed)
#pragma unroll
  for (int it = 0; it < kRdmLoads; ++it)
    if ((int)threadIdx.x + it * kBlock < S) tile[lidx[it]] = x[it];
  __syncthreads();
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
  rdm_thread_slots<R, true>(a, off, lidx);
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
__device__ __forceinline__ void rdm_block_of(int blk, int* I, int* J) {   // blocks of the lower triangle, row by row
  int i = 0;
  while ((i + 1) * (i + 2) / 2 <= blk) ++i;
  *I = i;
  *J = blk - i * (i + 1) / 2;
}

template <int R, bool NT>
__global__ __launch_bounds__(kBlock) void k_rdm_block(const RdmArgs a) {
  static_assert(R >= 4 && R <= kRdmMaxQubits, "4 x 4 blocks");
  constexpr int D = 1 << R, DB = D / 4, NB = DB * (DB + 1) / 2;
  constexpr int SL = R == 4 ? 16 : R == 5 ? 4 : 1;  // slices of e' per block: 160, 144, 136 threads at work
  static_assert(NB * SL <= kBlock, "a thread per (block, slice)");
  __shared__ double2 tile[kRdmTile];
  const int tid = threadIdx.x;
  const int eb = a.tb - R, E = 1 << eb;
  u64 off[kRdmLoads];
  int lidx[kRdmLoads];
  rdm_thread_slots<R, false>(a, off, lidx);
  const int blk = tid / SL, slice = tid % SL;
  const int sl = SL < E ? SL : E;                   // slices at work (small chunks: fewer e' than slices)
  const int L = E / sl;                             // e' per slice: slice + sl * 0 .. slice + sl * (L - 1)
  const bool active = blk < NB && slice < sl;
  int I = 0, J = 0;
  if (active) rdm_block_of(blk, &I, &J);
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
      int bi, bj;
      rdm_block_of(b, &bi, &bj);
      const double* r = red + v * kBlock + b * SL;
      double sum = r[0];
      for (int q = 1; q < SL; ++q) sum += r[q];
      const int x = 4 * bi + (v >> 2), y = 4 * bj + (v & 3);
      if (part == 0 ? x >= y : x > y) mine[part == 0 ? x * D + y : y * D + x] = sum;
    }
  }
}
#endif  // QSIM_PROBES

// (rdm_tile_row / rdm_tile_col, tile t = I (I + 1) / 2 + J of the lower triangle -> I, J: rdm_wide_plan.h)
// r = 6: wave W owns the units W, W + 4, .. (five of the twenty) over every k-step
template <int W, int NB>
__device__ __forceinline__ void rdm_mfma_own_units(const double (&p)[NB], const double (&q)[NB], qs_double4_t* acc) {
#pragma unroll
  for (int c = 0; c < 5; ++c) {
    constexpr int kWaves = kBlock / 64;
    const int u = W + kWaves * c, I = rdm_tile_row(u >> 1), J = rdm_tile_col(u >> 1);
    acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64((u & 1) ? q[I] : p[I], p[J], acc[c], 0, 0, 0);
  }
}
template <int W, int D>
__device__ __forceinline__ void rdm_mfma_store_units(const qs_double4_t* acc, double* mine, int j, int g) {
#pragma unroll
  for (int c = 0; c < 5; ++c) {
    constexpr int kWaves = kBlock / 64;
    const int u = W + kWaves * c, I = rdm_tile_row(u >> 1), J = rdm_tile_col(u >> 1);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int xr = 16 * I + 4 * i + g, yc = 16 * J + j;
      if (u & 1) { if (xr > yc) mine[yc * D + xr] = acc[c][i]; }
      else if (xr >= yc) mine[xr * D + yc] = acc[c][i];
    }
  }
}

template <int R, bool NT>
__global__ __launch_bounds__(kBlock) void k_rdm_mfma(const RdmArgs a) {
  static_assert(R >= 4 && R <= kRdmMaxQubits, "16 x 16 tiles");
  constexpr int D = 1 << R, NB = D / 16, NTILE = NB * (NB + 1) / 2, NU = 2 * NTILE;   // units: (tile, Re / Im)
  constexpr int kWaves = kBlock / 64;
  __shared__ double2 tile[kRdmTile + D];            // D rows of E + 1 words; later the waves' accumulators
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 15, g = lane >> 4;
  const int eb = a.tb - R, E = 1 << eb;
  u64 off[kRdmLoads];
  int lidx[kRdmLoads];
  rdm_thread_slots<R, false, true>(a, off, lidx);
  const int steps = E > 1 ? E >> 1 : 1;             // k-steps of two e' (E = 1: the second e' is a zero operand)
  const bool real_e = (g >> 1) < E;
  const bool im = g & 1;
  const double2* row = tile + j * (E + 1) + (real_e ? g >> 1 : 0);
  // r = 4, 5: every wave keeps all units and takes every fourth k-step; r = 6: all k-steps, a quarter of the units
  // (80 accumulator registers per unit set would leave one workgroup per CU)
  constexpr bool kOwnUnits = NU == 5 * kWaves;
  constexpr int NACC = kOwnUnits ? 5 : NU;
  constexpr int kStride = kOwnUnits ? 1 : kWaves;   // between the k-steps of a wave
  constexpr int kAhead = NB == 1 ? 4 : 1;           // r = 4: one LDS read feeds two MFMAs only, so four k-steps at a time
  qs_double4_t acc[NACC];
#pragma unroll
  for (int u = 0; u < NACC; ++u) acc[u] = qs_double4_t{0.0, 0.0, 0.0, 0.0};
  double2 nxt[kRdmLoads];                           // the tile on its way
  rdm_fetch<NT>(a, blockIdx.x, off, nxt);
  for (u64 o = blockIdx.x; o < a.n_tiles; o += gridDim.x) {
    rdm_stage(a, tile, lidx, nxt);
    rdm_fetch<NT>(a, o + gridDim.x, off, nxt);
    // kAhead k-steps at a time: their LDS reads are in flight before the first MFMA waits for one (r = 4: 4.85 -> 3.95 ms
    // at 30 qubits; r = 5 with two at a time drops to 3 waves per SIMD and gains nothing).  Steps beyond the last one,
    // in chunks of fewer amplitudes than a tile, are zero operands.
    for (int s0 = kOwnUnits ? 0 : wave; s0 < steps; s0 += kAhead * kStride) {
      double p[kAhead][NB], q[kAhead][NB];          // X and X' of the lane's row of every row block
#pragma unroll
      for (int n = 0; n < kAhead; ++n) {
        const int s = s0 + n * kStride;
        const bool use = real_e && s < steps;
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          const double2 v = row[(16 * b) * (E + 1) + 2 * (s < steps ? s : s0)];
          p[n][b] = use ? (im ? v.y : v.x) : 0.0;
          q[n][b] = use ? (im ? -v.x : v.y) : 0.0;
        }
      }
#pragma unroll
      for (int n = 0; n < kAhead; ++n) {
        if constexpr (kOwnUnits) {
          switch (wave) {
            case 0: rdm_mfma_own_units<0, NB>(p[n], q[n], acc); break;
            case 1: rdm_mfma_own_units<1, NB>(p[n], q[n], acc); break;
            case 2: rdm_mfma_own_units<2, NB>(p[n], q[n], acc); break;
            default: rdm_mfma_own_units<3, NB>(p[n], q[n], acc); break;
          }
        } else {
#pragma unroll
          for (int t = 0; t < NTILE; ++t) {
            acc[2 * t] = __builtin_amdgcn_mfma_f64_16x16x4f64(p[n][rdm_tile_row(t)], p[n][rdm_tile_col(t)], acc[2 * t], 0, 0, 0);
            acc[2 * t + 1] = __builtin_amdgcn_mfma_f64_16x16x4f64(q[n][rdm_tile_row(t)], p[n][rdm_tile_col(t)], acc[2 * t + 1], 0, 0, 0);
          }
        }
      }
    }
  }
  double* mine = a.partial + (u64)blockIdx.x * (D * D);
  if constexpr (kOwnUnits) {                        // a unit lives in one wave: straight from the accumulators
    switch (wave) {
      case 0: rdm_mfma_store_units<0, D>(acc, mine, j, g); break;
      case 1: rdm_mfma_store_units<1, D>(acc, mine, j, g); break;
      case 2: rdm_mfma_store_units<2, D>(acc, mine, j, g); break;
      default: rdm_mfma_store_units<3, D>(acc, mine, j, g); break;
    }
    return;
  }
  // the waves' accumulators in wave order, four units per round: red[unit of the round][wave][element i][lane]
  double* red = reinterpret_cast<double*>(tile);
  constexpr int kPerRound = 4;
  static_assert(kPerRound * kWaves * kBlock <= 2 * kRdmTile, "a round fits the tile");
#pragma unroll
  for (int u0 = 0; u0 < NU; u0 += kPerRound) {
    __syncthreads();
#pragma unroll
    for (int c = 0; c < kPerRound; ++c)
      if (u0 + c < NACC) {
#pragma unroll
        for (int i = 0; i < 4; ++i) red[((c * kWaves + wave) * 4 + i) * 64 + lane] = acc[u0 + c][i];
      }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < kPerRound; ++c)
      if (u0 + c < NU) {
        const int u = u0 + c, I = rdm_tile_row(u >> 1), J = rdm_tile_col(u >> 1);
        double sum = red[(c * kWaves) * kBlock + tid];            // thread tid = element tid >> 6 of lane tid & 63
        for (int w = 1; w < kWaves; ++w) sum += red[(c * kWaves + w) * kBlock + tid];
        const int xr = 16 * I + 4 * wave + g, yc = 16 * J + j;
        if (u & 1) { if (xr > yc) mine[yc * D + xr] = sum; }
        else if (xr >= yc) mine[xr * D + yc] = sum;
      }
  }
}

// ---- r = 7..12 (k_rdm_wide, qsim_reduced_density_matrix_wide; the host side is rdm_wide_plan.h)
// rho is cut into 64 x 64 blocks: six ROW qubits inside a block, r - 6 BLOCK qubits whose pattern I < NB names it.  A
// tile is staged exactly as k_rdm_mfma stages its r = 6 tile (64 rows of E words, row stride E + 1), with the block
// pattern deposited on the block qubits' physical bits.  Workgroup w = s * pairs + p takes the block pair p = (I, J),
// I >= J, and slice s of the outer tiles (s, s + S, ...): per outer tile it stages the tile of pattern I and, off the
// diagonal, the one of pattern J in a second LDS region, and accumulates Re = X_I X_J^T, Im = X'_I X_J^T.  Off the
// diagonal that is 16 MFMA tiles x 2 = 32 units: wave W owns row block W of I against the four column blocks of J, 8
// units, one LDS word of I and four of J per k-step.  On the diagonal it is the 20 units of the lower triangle, five per
// wave, as r = 6.  The workgroup writes its partial block (Re [a * 64 + b], Im at 4096 + the same; of a diagonal block
// only the tiles of the lower triangle) and k_hist_sum adds the slices in slice order.  No atomics.
static_assert(kRdmWideTileBits == kRdmTileBits && kRdmWideRowBits == kRdmMaxQubits, "the r = 6 staging serves the wide kernel");
constexpr int kRdmWideRegion = 64 * ((kRdmTile >> 6) + 1);   // words of one staged tile: 64 rows of E + 1

struct RdmWideArgs {
  RdmArgs t;                       // what rdm_thread_slots and rdm_fetch read: amp, the tile (tb, phys_bit, lds_pos), n_tiles = outer
                                   // tiles, outer_mask without the block qubits (its partial and swz stay unused: zero)
  double* partial;                 // [slice][pair][kRdmWideBlockDoubles]
  int blk_phys[kRdmWideMaxQubits - kRdmWideRowBits];   // block bit -> physical bit
  int nb_bits;
  int pairs;
  unsigned slices;
};

template <bool NT>
__global__ __launch_bounds__(kBlock) void k_rdm_wide(const RdmWideArgs a) {
  constexpr int kWaves = kBlock / 64;
  static_assert(kWaves == 4, "a wave per row block of 16");
  __shared__ double2 tile[2 * kRdmWideRegion];
  double2* const tile_i = tile;
  double2* const tile_j = tile + kRdmWideRegion;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 15, g = lane >> 4;
  const int eb = a.t.tb - 6, E = 1 << eb, tile_amps = 1 << a.t.tb;
  const int pair = (int)(blockIdx.x % (unsigned)a.pairs);
  const u64 slice = blockIdx.x / (unsigned)a.pairs;
  const int I = rdm_tile_row(pair), J = rdm_tile_col(pair);
  const bool diag = I == J;
  RdmArgs ai = a.t, aj = a.t;      // the two patterns' tiles: the deposit is disjoint from every other bit of an offset
  ai.amp += rdm_wide_deposit(a.blk_phys, a.nb_bits, I);
  aj.amp += rdm_wide_deposit(a.blk_phys, a.nb_bits, J);
  u64 off[kRdmLoads];
  int lidx[kRdmLoads];
  rdm_thread_slots<6, false, true>(a.t, off, lidx);
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
  for (u64 o = slice; o < a.t.n_tiles; o += a.slices) {
    __syncthreads();                                // (the previous tiles are consumed)
#pragma unroll
    for (int it = 0; it < kRdmLoads; ++it)
      if (tid + it * kBlock < tile_amps) {
        tile_i[lidx[it]] = nxt_i[it];
        if (!diag) tile_j[lidx[it]] = nxt_j[it];
      }
    __syncthreads();
    rdm_fetch<NT>(ai, o + a.slices, off, nxt_i);
    if (!diag) rdm_fetch<NT>(aj, o + a.slices, off, nxt_j);
    if (diag) {
      const double2* row = tile_i + row_off;
      for (int s = 0; s < steps; ++s) {
        double p[4], q[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const double2 v = row[(16 * b) * (E + 1) + 2 * s];
          p[b] = real_e ? (im ? v.y : v.x) : 0.0;
          q[b] = real_e ? (im ? -v.x : v.y) : 0.0;
        }
        switch (wave) {
          case 0: rdm_mfma_own_units<0, 4>(p, q, acc); break;
          case 1: rdm_mfma_own_units<1, 4>(p, q, acc); break;
          case 2: rdm_mfma_own_units<2, 4>(p, q, acc); break;
          default: rdm_mfma_own_units<3, 4>(p, q, acc); break;
        }
      }
    } else {
      const double2* row_i = tile_i + row_off + (16 * wave) * (E + 1);
      const double2* row_j = tile_j + row_off;
      for (int s = 0; s < steps; ++s) {
        const double2 u = row_i[2 * s];
        const double pi = real_e ? (im ? u.y : u.x) : 0.0;
        const double qi = real_e ? (im ? -u.x : u.y) : 0.0;
        double pj[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const double2 v = row_j[(16 * b) * (E + 1) + 2 * s];
          pj[b] = real_e ? (im ? v.y : v.x) : 0.0;
        }
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
#pragma unroll
    for (int c = 0; c < 5; ++c) {
      const int u = wave + kWaves * c;              // the unit numbering of rdm_mfma_own_units
      const int ti = rdm_tile_row(u >> 1), tj = rdm_tile_col(u >> 1);
#pragma unroll
      for (int i = 0; i < 4; ++i) mine[(u & 1) * 4096 + (16 * ti + 4 * i + g) * 64 + 16 * tj + j] = acc[c][i];
    }
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
