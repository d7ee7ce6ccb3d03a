// dense_kernels.h -- the dense k-qubit block (qsim_apply_fused_k, k = 3 .. 6): the kernels on the matrix cores, the LDS
// form for tiny chunks, the probe build's earlier forms, and the launcher.
// Part of the single translation unit qsim_hip.hip (included there, in order; not a standalone header).
typedef double qs_double4_t __attribute__((ext_vector_type(4)));      // the accumulator of v_mfma_f64_16x16x4_f64

#ifdef QSIM_PROBES         // (the vector-ALU form and the round-4 MFMA form: kept in the probe build as A/B partners of k_dense_mfma2 below)
// ---- dense k-qubit block (v3's fused block as a genuine 2^k x 2^k contraction: parallel_gate_applicator.py:315-385) ------
// A work item owns the 2^K amplitudes that differ in the block's K index bits; new = M old with M row-major in device
// memory (wave-uniform addresses: scalar loads).  HBM-bound like every gate here (8 * 2^K flop per amplitude over the
// same 32 B: 2 flop / B at K = 3, 4 at K = 4 -- far under the fp64 ridge); the matrix cores would pay from K ~ 5-6 on
// (tools/mfma_probe.hip), which no caller of the reference's gate set produces.
struct DenseArgs {
  double2* amp;
  const double2* mat;       // 2^K x 2^K, row-major: M[out][in]
  u64 count;                // work items = 2^(k - K)
  int pos[4];               // the block's index bits, ascending (zeros are inserted there)
  int bit[4];               // pattern bit i <-> index bit bit[i] (the caller's qubit order)
};
template <int K, bool NT>
__global__ __launch_bounds__(kBlock) void k_dense(const DenseArgs a) {
  constexpr int N = 1 << K;
  u64 c = logical_block<true>() * kBlock + threadIdx.x;
  if (c >= a.count) return;
#pragma unroll
  for (int i = 0; i < K; ++i) { const int p = a.pos[i]; c = ((c >> p) << (p + 1)) | (c & ((1ull << p) - 1)); }
  double2 x[N];
#pragma unroll
  for (int s = 0; s < N; ++s) {
    u64 off = 0;
#pragma unroll
    for (int i = 0; i < K; ++i) off |= (u64)((s >> i) & 1) << a.bit[i];
    x[s] = ld_amp<NT>(a.amp + (c | off));
  }
#pragma unroll
  for (int r = 0; r < N; ++r) {
    double2 acc = cmul(a.mat[r * N], x[0]);
#pragma unroll
    for (int col = 1; col < N; ++col) acc = cfma(a.mat[r * N + col], x[col], acc);
    u64 off = 0;
#pragma unroll
    for (int i = 0; i < K; ++i) off |= (u64)((r >> i) & 1) << a.bit[i];
    st_amp<NT>(a.amp + (c | off), acc);
  }
}

// Dense 3- and 4-qubit blocks on the MATRIX cores (round 4): a genuine 2^K x 2^K complex contraction per block of 2^K
// amplitudes = a real 2^(K+1) x 2^(K+1) matrix [[Re, -Im], [Im, Re]] (rows / columns 2 p + c: pattern p, c = 0 real / 1
// imaginary -- the order the amplitudes lie in memory) times the 2^(K+1) reals of the block, as v_mfma_f64_16x16x4_f64: a
// wave takes 16 COLUMNS (= 16 blocks: consecutive values of the index bits that are not block bits) at a time; K = 4: two
// 16-row output tiles x eight k-steps = 16 MFMAs per 256 amplitudes (128 flop per amplitude: 1.75 ms of the matrix cores'
// 78 Tflop/s at 30 qubits, under the 4.3 ms of HBM); K = 3: one tile x four k-steps per 128 amplitudes.  Operand layouts
// (lane l: j = l & 15, g = l >> 4; measured with tools/mfma_probe.hip in round 2):
//   A of k-step s, row tile t:  Mr[16 t + j][4 s + g]            (formed once per wave from the caller's complex matrix)
//   B of k-step s:              X[row 4 s + g][column j]  = component g & 1 of pattern 2 s + (g >> 1) of block j
//   D element i of row tile t:  Y[row 16 t + 4 i + g][column j] = component g & 1 of pattern 2 (4 t + i) + (g >> 1)
// so a lane reads the doubles { pattern 2 m + (g >> 1), m = 0 .. 2^(K-1) - 1 } x { component g & 1 } of its block and writes
// its results back to the same places: in place, no shuffles, no LDS.  Lane pairs (g & 1) cover one amplitude (16 B), 32
// lanes 256 contiguous bytes when the block bits lie above index bit 3.  Measured at 30 qubits (profiles/r04x_*): K = 4
// 0.68-0.73 of the HBM peak against 0.43 for the vector-ALU form (k_dense<4>: 256 complex multiply-adds per work item at 128+
// VGPRs) -- the one place of this path where the work IS a matrix product (north star: "MFMA only for fused
// multi-qubit dense blocks where it is a real 2^k x 2^k contraction").
struct DenseMfmaArgs {
  double* amp;              // the chunk as reals
  const double2* mat;       // the caller's 2^K x 2^K complex matrix, row-major M[out][in] (its real image is formed in registers)
  u64 col_blocks;           // groups of 16 columns: 2^(k - K - 4)
  int pos[4];               // the block's index bits, ascending (zeros are inserted there)
  int bit[4];               // pattern bit i <-> index bit bit[i] (the caller's qubit order)
};
constexpr int kDenseMfmaColBlocksPerWave = 4;
template <int K, bool NT>
__global__ __launch_bounds__(kBlock) void k_dense_mfma(const DenseMfmaArgs a) {
  static_assert(K == 3 || K == 4, "16-row MFMA tiles: 16 or 32 reals per block");
  constexpr int TT = 1 << (K - 3);          // 16-row output tiles
  constexpr int S = 1 << (K - 1);           // k-steps of 4 rows = patterns per lane
  constexpr int DIM = 1 << K;
  const int l = threadIdx.x & 63, j = l & 15, g = l >> 4;
  double A[TT][S];
#pragma unroll
  for (int t = 0; t < TT; ++t)
#pragma unroll
    for (int s = 0; s < S; ++s) {
      // Mr[2 po + co][2 pi + ci] = Re M[po][pi] if co == ci, Im if (co, ci) = (1, 0), -Im if (0, 1)
      const int r = 16 * t + j, col = 4 * s + g;
      const double2 z = a.mat[(r >> 1) * DIM + (col >> 1)];
      A[t][s] = (r & 1) == (col & 1) ? z.x : ((r & 1) ? z.y : -z.y);
    }
  u64 off[S];               // (wave-uniform) offsets of the patterns' upper K - 1 bits, in reals
#pragma unroll
  for (int m = 0; m < S; ++m) {
    u64 o = 0;
#pragma unroll
    for (int i = 0; i < K - 1; ++i) o |= (u64)((m >> i) & 1) << a.bit[i + 1];
    off[m] = 2 * o;
  }
  const u64 lane_part = 2 * ((u64)(g >> 1) << a.bit[0]) + (u64)(g & 1);
  const u64 wave = logical_block<true>() * (kBlock / 64) + (threadIdx.x >> 6);
#pragma unroll
  for (int it = 0; it < kDenseMfmaColBlocksPerWave; ++it) {
    const u64 cb = wave * kDenseMfmaColBlocksPerWave + it;
    if (cb >= a.col_blocks) break;                    // (wave-uniform)
    u64 c = cb * 16 + (u64)j;
#pragma unroll
    for (int i = 0; i < K; ++i) { const int p = a.pos[i]; c = ((c >> p) << (p + 1)) | (c & ((1ull << p) - 1)); }
    double* const p0 = a.amp + 2 * c + lane_part;
    double x[S];
#pragma unroll
    for (int m = 0; m < S; ++m) x[m] = NT ? __builtin_nontemporal_load(p0 + off[m]) : p0[off[m]];
    qs_double4_t acc[TT];
#pragma unroll
    for (int t = 0; t < TT; ++t) acc[t] = qs_double4_t{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int s = 0; s < S; ++s)
#pragma unroll
      for (int t = 0; t < TT; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(A[t][s], x[s], acc[t], 0, 0, 0);
#pragma unroll
    for (int t = 0; t < TT; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (NT) __builtin_nontemporal_store(acc[t][i], p0 + off[4 * t + i]);
        else p0[off[4 * t + i]] = acc[t][i];
      }
  }
}

#endif  // QSIM_PROBES

// Dense K-qubit blocks, K = 3 .. 6, on the matrix cores -- second form (round 5).  Same product as k_dense_mfma (a real
// 2^(K+1) x 2^(K+1) matrix times the reals of 16 blocks per wave and step, v_mfma_f64_16x16x4_f64), with two changes:
//   * the ROWS are ordered so that a lane owns WHOLE amplitudes: row r = 4 s + g with s = 2 mu + c -- g = the two LOWEST
//     pattern bits (the block's two lowest index bits), c = component (0 real, 1 imaginary), mu = the upper K - 2 pattern
//     bits.  Lane (j = l & 15, g = l >> 4) then holds the 2^(K-2) amplitudes { pattern 4 mu + g } of column j as double2 and
//     gets them back at the same places (D element i of row tile t is row 16 t + 4 i + g: s' = 4 t + i): 16-byte accesses,
//     in place, no LDS for the state, no shuffles.  With the block's lowest bits inside a 128-byte line the four g lanes of
//     a column cover 64 contiguous bytes and two neighbouring columns the rest of the line (r04's form touched every line
//     with four 32-byte pieces: 0.40 of peak on blocks over index bits 0-2);
//   * K = 5 and 6: the matrix image no longer fits registers (16 x 2^(K-1) / 64 ... = 64 / 256 doubles per lane), so every
//     workgroup keeps it in LDS in A-OPERAND layout -- tab[(t S + s) 64 + lane] = Mr[16 t + (lane & 15)][4 s + (lane >> 4)],
//     32 / 128 KiB -- and each MFMA takes its A operand with one conflict-free ds_read_b64.  K = 6 is the first kernel of
//     this path that is NOT bound by HBM: 512 flop per amplitude = 7.0 ms of the 78.6 Tflop/s at 30 qubits against 4.3 ms
//     of HBM at peak (K = 5: 3.5 ms against 4.3: HBM still).
// Mr[(mu_o, c_o, g_o)][(mu_i, c_i, g_i)] = Re M[p_o][p_i] if c_o == c_i, Im if (c_o, c_i) = (1, 0), -Im if (0, 1), with
// p = 4 mu + g in SORTED block-bit order; `to_caller[i]` = the caller's pattern bit of the i-th lowest block bit.
struct DenseMfma2Args {
  double2* amp;
  const double2* mat;       // the caller's 2^K x 2^K complex matrix, row-major M[out][in]
  u64 col_blocks;           // groups of 16 columns: 2^(k - K - 4)
  int pos[6];               // the block's index bits, ascending
  int to_caller[6];         // pattern bit i (sorted order) -> bit of the caller's pattern
  int consec_log2;          // a wave takes runs of 2^consec_log2 CONSECUTIVE column groups (its accesses to one pattern then
                            // cover 2^consec_log2 x 256 contiguous bytes over as many steps), run after run strided through its XCD's region
  u64 skew;                 // (probe knob) XCD x starts x * skew column groups into its region (wrapping): the eight streams out of step
};
template <int K>
__device__ __forceinline__ double dense_mr_entry(const DenseMfma2Args& a, int t, int s, int lane) {
  const int j = lane & 15, g = lane >> 4;
  const int so = 4 * t + (j >> 2), go = j & 3;
  const int po = 4 * (so >> 1) + go, co = so & 1, pi = 4 * (s >> 1) + g, ci = s & 1;
  int ro = 0, ri = 0;
#pragma unroll
  for (int i = 0; i < K; ++i) { ro |= ((po >> i) & 1) << a.to_caller[i]; ri |= ((pi >> i) & 1) << a.to_caller[i]; }
  const double2 z = a.mat[ro * (1 << K) + ri];
  return co == ci ? z.x : (co ? z.y : -z.y);
}
// PF: how the NEXT column group's amplitudes are requested.  1: before this group's products, if there is a next group --
// the compiler's waits must then cover the case without one, and in the steady state the first MFMA waits for the loads
// just requested: the overlap is left to the other waves of the SIMD.  Measured best for K <= 5: what bounds them is the
// memory system's rate for this access shape, and MORE bytes in flight lower it (a true prefetch costs K = 3, 4 3-15 %).
// 2: requested UNCONDITIONALLY (a wave's last group asks for itself again, unused) after one explicit wait for the first
// group's loads: no wait in the MFMA chain, the loads land behind it (K = 6, bound by the matrix cores with 2 waves per
// SIMD: -3 %).  0 (probe build): not ahead at all.  profiles/r05q_dense_knob_scans.txt
template <int K, bool NT, int THREADS, int PF>
__global__ __launch_bounds__(THREADS) void k_dense_mfma2(const DenseMfma2Args a) {
  static_assert(K >= 3 && K <= 6, "dense blocks of 3 .. 6 qubits");
  constexpr int TT = 1 << (K - 3);          // 16-row output tiles
  constexpr int S = 1 << (K - 1);           // k-steps of 4 rows
  constexpr int MU = 1 << (K - 2);          // amplitudes per lane and column
  constexpr bool IN_LDS = K >= 5;
  __shared__ double tab[IN_LDS ? TT * S * 64 : 1];
  const int l = threadIdx.x & 63, j = l & 15, g = l >> 4;
  double A[IN_LDS ? 1 : TT][IN_LDS ? 1 : S];
  if constexpr (IN_LDS) {
    for (int idx = threadIdx.x; idx < TT * S * 64; idx += THREADS) tab[idx] = dense_mr_entry<K>(a, idx / (S * 64), (idx >> 6) % S, idx & 63);
    __syncthreads();
  } else {
#pragma unroll
    for (int t = 0; t < TT; ++t)
#pragma unroll
      for (int s = 0; s < S; ++s) A[t][s] = dense_mr_entry<K>(a, t, s, l);
  }
  u64 off[MU];              // (wave-uniform) offsets of the upper pattern bits, in amplitudes
#pragma unroll
  for (int m = 0; m < MU; ++m) {
    u64 o = 0;
#pragma unroll
    for (int i = 0; i < K - 2; ++i) o |= (u64)((m >> i) & 1) << a.pos[i + 2];
    off[m] = o;
  }
  const u64 lane_part = ((u64)(g & 1) << a.pos[0]) | ((u64)(g >> 1) << a.pos[1]);
  // Column groups of a wave: the workgroups are dealt round-robin over the 8 XCDs, so workgroup b works in the b % 8-th
  // contiguous eighth of the column groups (one XCD's L2 sees one region) and the waves of an XCD stride through it.
  const u64 bid = (u64)blockIdx.y * gridDim.x + blockIdx.x, n_blocks = (u64)gridDim.x * gridDim.y;
  const bool split = (n_blocks & 7) == 0 && (a.col_blocks & 7) == 0;
  const u64 region = split ? a.col_blocks >> 3 : a.col_blocks;
  const u64 region_base = split ? (bid & 7) * region : 0;
  const u64 wave_in_region = (split ? bid >> 3 : bid) * (THREADS / 64) + (threadIdx.x >> 6);          // (wave-uniform)
  const u64 run = 1ull << a.consec_log2;
  const u64 run_stride = ((split ? n_blocks >> 3 : n_blocks) * (THREADS / 64) - 1) << a.consec_log2;   // from a run's end to the wave's next run
  u64 cb = wave_in_region << a.consec_log2;
  const u64 rot = split ? ((bid & 7) * a.skew) % region : 0;
  auto column_ptr = [&](u64 col_block) -> double2* {
    u64 cr = col_block + rot;
    if (cr >= region) cr -= region;
    u64 c = (region_base + cr) * 16 + (u64)j;
#pragma unroll
    for (int i = 0; i < K; ++i) { const int p = a.pos[i]; c = ((c >> p) << (p + 1)) | (c & ((1ull << p) - 1)); }
    return a.amp + (c | lane_part);
  };
  if (cb >= region) return;
  double2* p0 = column_ptr(cb);
  double2 x[MU];
#pragma unroll
  for (int m = 0; m < MU; ++m) x[m] = ld_amp<NT>(p0 + off[m]);
  if constexpr (PF == 2) __builtin_amdgcn_s_waitcnt(0x0f70);       // vmcnt(0), the other counters left alone (once per wave)
  for (;;) {
    const u64 cb_next = ((cb + 1) & (run - 1)) ? cb + 1 : cb + 1 + run_stride;
    const bool more = cb_next < region;               // (wave-uniform)
    double2* const p1 = more ? column_ptr(cb_next) : p0;
    double2 xn[MU];
    if (PF == 2 || (PF == 1 && more)) {
#pragma unroll
      for (int m = 0; m < MU; ++m) xn[m] = ld_amp<NT>(p1 + off[m]);
    }
    qs_double4_t acc[TT];
#pragma unroll
    for (int t = 0; t < TT; ++t) acc[t] = qs_double4_t{0.0, 0.0, 0.0, 0.0};
    if constexpr (IN_LDS) {
      // A operands from LDS, one k-step ahead of the MFMAs that use them; the scheduling barrier keeps the compiler from
      // hoisting all TT x S reads to the top (it did: 256 VGPRs and 368 spilled at K = 6)
      double cur[TT], nxt[TT];
#pragma unroll
      for (int t = 0; t < TT; ++t) cur[t] = tab[(t * S) * 64 + l];
#pragma unroll
      for (int s = 0; s < S; ++s) {
        if (s + 1 < S) {
#pragma unroll
          for (int t = 0; t < TT; ++t) nxt[t] = tab[(t * S + s + 1) * 64 + l];
        }
        const double b = (s & 1) ? x[s >> 1].y : x[s >> 1].x;
#pragma unroll
        for (int t = 0; t < TT; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(cur[t], b, acc[t], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int t = 0; t < TT; ++t) cur[t] = nxt[t];
      }
    } else {
#pragma unroll
      for (int s = 0; s < S; ++s) {
        const double b = (s & 1) ? x[s >> 1].y : x[s >> 1].x;
#pragma unroll
        for (int t = 0; t < TT; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(A[IN_LDS ? 0 : t][IN_LDS ? 0 : s], b, acc[t], 0, 0, 0);
      }
    }
#pragma unroll
    for (int t = 0; t < TT; ++t)
#pragma unroll
      for (int h = 0; h < 2; ++h) st_amp<NT>(p0 + off[2 * t + h], make_double2(acc[t][2 * h], acc[t][2 * h + 1]));
    if (!more) break;
    cb = cb_next;
    p0 = p1;
    if constexpr (PF == 0) {
#pragma unroll
      for (int m = 0; m < MU; ++m) x[m] = ld_amp<NT>(p0 + off[m]);
    } else {
#pragma unroll
      for (int m = 0; m < MU; ++m) x[m] = xn[m];
    }
  }
}

template <int K> constexpr int kDensePf = K == 6 ? 2 : 1;       // the product's choice per K (see PF above)
template <int K, bool NT, int THREADS>
static void launch_dense_mfma2(const DenseMfma2Args& d, unsigned grid, hipStream_t stream, int pf) {
#ifdef QSIM_PROBES
  if (pf == 0) { hipLaunchKernelGGL((k_dense_mfma2<K, NT, THREADS, 0>), dim3(grid), dim3(THREADS), 0, stream, d); return; }
  if (pf == 1) { hipLaunchKernelGGL((k_dense_mfma2<K, NT, THREADS, 1>), dim3(grid), dim3(THREADS), 0, stream, d); return; }
  if (pf == 2) { hipLaunchKernelGGL((k_dense_mfma2<K, NT, THREADS, 2>), dim3(grid), dim3(THREADS), 0, stream, d); return; }
#endif
  (void)pf;
  hipLaunchKernelGGL((k_dense_mfma2<K, NT, THREADS, kDensePf<K>>), dim3(grid), dim3(THREADS), 0, stream, d);
}

// Chunks too small for 16 columns per wave (fewer than 2^(K+4) amplitudes): one 64-thread workgroup per block, the block's
// 2^K amplitudes through LDS.  Correctness path for tiny chunks (tests, chunked runners with small chunk_size).
struct DenseSmallArgs {
  double2* amp;
  const double2* mat;
  int k;
  int pos[6];
  int bit[6];
};
__global__ __launch_bounds__(64) void k_dense_small(const DenseSmallArgs a) {
  __shared__ double2 x[64];
  const int N = 1 << a.k;
  u64 c = blockIdx.x;
  for (int i = 0; i < a.k; ++i) { const int p = a.pos[i]; c = ((c >> p) << (p + 1)) | (c & ((1ull << p) - 1)); }
  const int r = threadIdx.x;
  u64 off = 0;
  for (int i = 0; i < a.k; ++i) off |= (u64)((r >> i) & 1) << a.bit[i];
  if (r < N) x[r] = a.amp[c | off];
  __syncthreads();
  if (r < N) {
    double2 acc = cmul(a.mat[r * N], x[0]);
    for (int col = 1; col < N; ++col) acc = cfma(a.mat[r * N + col], x[col], acc);
    a.amp[c | off] = acc;
  }
}

// The launcher: what qsim_apply_fused_k does with a checked block of k = 3 .. 6 distinct local qubits (the matrix goes to the
// chunk's scratch).
static int apply_dense_block(qsim_chunk* c, int k, const int32_t* qubits, const double* M) {
  HIP_TRY(hipSetDevice(c->device));
  const int rc = ensure_scratch(c);
  if (rc) return rc;
  const int N = 1 << k;
  static_assert(kScratchDoubles * sizeof(double) >= 64 * 64 * sizeof(double2), "the chunk's scratch holds a 64 x 64 complex matrix");
  HIP_TRY(hipMemcpyAsync(c->scratch, M, sizeof(double2) * (size_t)N * N, hipMemcpyHostToDevice, c->stream));
  int sorted[6] = {0, 0, 0, 0, 0, 0};
  for (int i = 0; i < k; ++i) sorted[i] = qubits[i];
  std::sort(sorted, sorted + k);
  const bool nt = c->span_bytes > tuning().mall_bytes && sorted[0] >= kLaneCut;
#ifdef QSIM_PROBES
  if (k <= 4 && tuning().dense_form == 0) {          // the round-4 kernels, kept in the probe build as A/B partners
    DenseArgs a;
    a.amp = c->amp;
    a.mat = reinterpret_cast<const double2*>(c->scratch);
    a.count = amps(c) >> k;
    for (int i = 0; i < 4; ++i) { a.bit[i] = i < k ? qubits[i] : 0; a.pos[i] = i < k ? sorted[i] : 0; }
    ProfileScope prof(kClsDense, 32.0 * (double)amps(c), c->stream, nt);
    if (c->k >= k + 4 && ((tuning().dense_mfma >> (k - 3)) & 1)) {
      DenseMfmaArgs d;
      d.amp = reinterpret_cast<double*>(c->amp);
      d.mat = a.mat;
      d.col_blocks = amps(c) >> (k + 4);
      for (int i = 0; i < 4; ++i) { d.pos[i] = a.pos[i]; d.bit[i] = a.bit[i]; }
      const u64 waves = (d.col_blocks + kDenseMfmaColBlocksPerWave - 1) / kDenseMfmaColBlocksPerWave;
      u64 wgs = (waves + kBlock / 64 - 1) / (kBlock / 64);
      wgs = (wgs + 7) & ~7ull;
      if (k == 3) QSIM_WITH_NT(hipLaunchKernelGGL((k_dense_mfma<3, NT>), grid_for(wgs), dim3(kBlock), 0, c->stream, d));
      else QSIM_WITH_NT(hipLaunchKernelGGL((k_dense_mfma<4, NT>), grid_for(wgs), dim3(kBlock), 0, c->stream, d));
    } else {
      u64 blocks = (a.count + kBlock - 1) / kBlock;
      blocks = (blocks + 7) & ~7ull;
      if (k == 3) QSIM_WITH_NT(hipLaunchKernelGGL((k_dense<3, NT>), grid_for(blocks), dim3(kBlock), 0, c->stream, a));
      else QSIM_WITH_NT(hipLaunchKernelGGL((k_dense<4, NT>), grid_for(blocks), dim3(kBlock), 0, c->stream, a));
    }
  } else
#endif
  {
    ProfileScope prof(kClsDense, 32.0 * (double)amps(c), c->stream, nt);
    if (c->k >= k + 4) {
      DenseMfma2Args d;
      d.amp = c->amp;
      d.mat = reinterpret_cast<const double2*>(c->scratch);
      d.col_blocks = amps(c) >> (k + 4);
      d.consec_log2 = 0;
      d.skew = 0;
      for (int i = 0; i < 6; ++i) {
        d.pos[i] = i < k ? sorted[i] : 0;
        d.to_caller[i] = 0;
        for (int q = 0; q < k; ++q) if (i < k && qubits[q] == sorted[i]) d.to_caller[i] = q;
      }
      // k <= 4: a wave takes four CONSECUTIVE column groups (the matrix image costs a few loads per wave; 64 columns = 1 KiB
      // contiguous per pattern over its four steps: -3 / -5 % against groups strided through the region, the worst
      // placements -8 / -13 %); k = 5, 6: resident workgroups that walk the column groups (the image is built once per
      // workgroup in LDS: 32 / 128 KiB) -- for k = 5 TWO per CU, not the four that fit: fewer bytes in flight suit the
      // memory system better (-9 %; one per CU is as good, three and four are not).  profiles/r05q_dense_knob_scans.txt
      int cus = 256;
      (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device);
      int pf = -1, groups = 4, wgs_per_cu = 2, consec_log2 = k <= 4 ? 2 : 0;       // (pf: the product's choice per k, kDensePf)
#ifdef QSIM_PROBES
      if (tuning().dense_pf >= 0) pf = tuning().dense_pf;
      if (tuning().dense_groups > 0) groups = tuning().dense_groups;
      if (tuning().dense_wgs > 0) wgs_per_cu = tuning().dense_wgs;
      if (tuning().dense_consec > 0) { consec_log2 = 0; while ((2 << consec_log2) <= tuning().dense_consec) ++consec_log2; }
      d.skew = (u64)tuning().dense_skew;
#endif
      d.consec_log2 = consec_log2;
      if (k <= 4) {
        const u64 waves = (d.col_blocks + groups - 1) / groups;
        const unsigned grid = (unsigned)std::min<u64>(((std::max<u64>((waves + 3) / 4, 1) + 7) & ~7ull), 1u << 20);   // (whole octets: one region per XCD)
        if (k == 3) QSIM_WITH_NT(launch_dense_mfma2<3, NT, 256>(d, grid, c->stream, pf));
        else QSIM_WITH_NT(launch_dense_mfma2<4, NT, 256>(d, grid, c->stream, pf));
      } else if (k == 5) {
        const unsigned grid = (unsigned)std::min<u64>((std::max<u64>((d.col_blocks + 3) / 4, 1) + 7) & ~7ull, (u64)cus * wgs_per_cu);
        QSIM_WITH_NT(launch_dense_mfma2<5, NT, 256>(d, grid, c->stream, pf));
      } else {
        const unsigned grid = (unsigned)std::min<u64>((std::max<u64>((d.col_blocks + 7) / 8, 1) + 7) & ~7ull, (u64)cus);
        QSIM_WITH_NT(launch_dense_mfma2<6, NT, 512>(d, grid, c->stream, pf));
      }
    } else {
      DenseSmallArgs a;
      a.amp = c->amp;
      a.mat = reinterpret_cast<const double2*>(c->scratch);
      a.k = k;
      for (int i = 0; i < 6; ++i) { a.bit[i] = i < k ? qubits[i] : 0; a.pos[i] = i < k ? sorted[i] : 0; }
      hipLaunchKernelGGL(k_dense_small, dim3((unsigned)(amps(c) >> k)), dim3(64), 0, c->stream, a);
    }
  }
  HIP_TRY(hipGetLastError());
  return QSIM_OK;
}
