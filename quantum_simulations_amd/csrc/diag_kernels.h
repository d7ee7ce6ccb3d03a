// diag_kernels.h -- diagonal Pauli sums D = sum_t c_t Z^{z_t}: the phase exp(-i gamma D) and the moments <D>, <D^2>
// (qsim_apply_diagonal_phase, qsim_diagonal_moments), and D as an operator: dst (+)= D src and <bra|ket>, <bra|D|ket>
// (qsim_apply_diagonal_sum, qsim_overlap_diagonal), and the values of the single terms <Z^{z_t}> (qsim_expectation_z_terms,
// k_diag_term_values below).
// Part of the single translation unit qsim_hip.hip (included there after rot_kernels.h; not a standalone header).
//
// E(i) = sum_t c_t (-1)^popcount(i & z_t) is the diagonal entry of D at index i.  D moves no amplitude, so a tile is the
// 2^tb CONTIGUOUS amplitudes on the lowest tb = min(k, kExpTileBits) index bits (no TileWalk), base = o << tb.  With the
// outer bits fixed,   E(base | j) = sum_m W[m] (-1)^popcount(j & m),   W[m] = sum_{t: zi_t = m} c_t (-1)^popcount(base & zo_t):
// E over the tile is the Walsh-Hadamard transform of the sparse spectrum W (tables and summation order: diag_plan.h).
// Per tile (diag_tiles below, the loop of k_diag_tile, k_diag_apply and k_diag_overlap: one workgroup per tile in a
// grid-stride loop):
//   1. the thread's kExpLoads amplitudes j = tid + it * kBlock are loaded into REGISTERS and stay there (tile_load's
//      slots): the LDS of a workgroup is W (16 KiB) and the piece slots (8 KiB), 24 KiB against the 32 KiB tile of the
//      other Pauli passes, so four workgroups per CU fit with room to spare, and the loads are in flight during 2. and 3.;
//   2. W is built: a thread per piece (kDiagPiece terms in table order, one __popcll(base & zo) each), then a thread per
//      join.  Pieces are dealt to LANES, so these table reads are per-lane loads (through the constant address space;
//      consecutive lanes read consecutive pieces); only the launch arguments are wave-uniform.  No atomics;
//   3. the transform, unscaled (it IS E), always over all kExpTileBits bits -- for a chunk of fewer bits W is zero
//      above 2^tb and E(j) repeats -- in four rounds of register butterflies: bits 0-2, 3-5, 6-7 through LDS with a
//      __syncthreads() between rounds, bits 8-10 on the thread's own slots tid + r * kBlock, which leaves E(j) in
//      registers next to amplitude j.  The last round zeroes what it reads: W is clear for the next tile;
//   4. the kernel's own lines, body(base, x, e):
//      phase:   psi_j *= cos(gamma E_j) - i sin(gamma E_j) (diag_sincos), stored back in place (tiles partition the
//      index space);
//      moments: p = |psi_j|^2 into the thread's running sums of p, p E, p E^2 over its slots and tiles; at the end lane
//      tree -> waves in wave order -> the workgroup's row of partials (block_sum_row); k_hist_sum adds the rows in
//      workgroup order;
//      sum (k_diag_apply):       dst_j = E_j src_j, or dst_j += E_j src_j: E is a multiplier, not an angle;
//      overlap (k_diag_overlap): q = conj(bra_j) ket_j into running sums of q and q E_j (re, im), reduced like the moments.
//      The second operand of these two (dst when accumulating, bra) is loaded AFTER the transform: its 8 double2 are
//      not alive next to src / ket during the rounds.
// The cost per tile is T term reads, 11 add/sub stages and one sincos per amplitude: nearly independent of T
// (profiles/r22_diagonal_probe.json).
constexpr int kDiagPhase = 0, kDiagMoments = 1;

struct DiagArgs {
  double2* amp;          // phase, moments: the chunk; sum: src; overlap: ket -- loaded before the transform
  double2* other;        // sum: dst; overlap: bra -- touched after the transform only
  const DiagTerm* terms;
  const DiagPiece* pieces;
  const DiagJoin* joins;
  double* partial;       // moments: [workgroup][3]; overlap: [workgroup][4]
  u64 n_tiles;           // 2^(k - tb)
  double gamma;          // phase
  int tb;                // tile bits: min(k, kExpTileBits)
  int n_pieces, n_joins;
};

// the butterflies of NB stages over 2^NB values in registers
template <int NB>
__device__ __forceinline__ void diag_butterflies(double* v) {
#pragma unroll
  for (int s = 0; s < NB; ++s)
#pragma unroll
    for (int i = 0; i < (1 << NB); ++i)
      if (!((i >> s) & 1)) {
        const double p = v[i], q = v[i | (1 << s)];
        v[i] = p + q;
        v[i | (1 << s)] = p - q;
      }
}

// stages B .. B + NB - 1 of the transform in LDS: the thread's kExpLoads entries as kExpLoads >> NB groups of 2^NB
template <int B, int NB>
__device__ __forceinline__ void diag_round(double* W) {
  constexpr int G = kExpLoads >> NB;
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const int u = (int)threadIdx.x * G + g;
    const int j0 = (u & ((1 << B) - 1)) | ((u >> B) << (B + NB));
    double v[1 << NB];
#pragma unroll
    for (int r = 0; r < (1 << NB); ++r) v[r] = W[j0 | (r << B)];
    diag_butterflies<NB>(v);
#pragma unroll
    for (int r = 0; r < (1 << NB); ++r) W[j0 | (r << B)] = v[r];
  }
}

// cos(v), sin(v) for any finite v: the angle in turns, r = v / (2 pi) - rint(v / (2 pi)) with 1 / (2 pi) as a double-double
// (the fma keeps the product exact before the subtraction, so |r| <= 1/2 carries an error of about 1 ulp for the
// |v| of a cost layer), then sincospi(2 r), which has no large-argument path: with sincos(v) the kernel took 140 VGPRs
// and spilled 18 of them at the 128 of four workgroups per CU, with this form 132 and 5 (round 22; with the build of W
// and the rounds in diag_energies the compiler now reports 128 and no spill).  k_diag_tile asks for the four
// (amdgpu_waves_per_eu): left at 132 VGPRs and three workgroups per CU the phase pass measured 4 % slower at 8 terms
// and 26 % slower at 4096 (profiles/r22_diagonal_ab.json).
__device__ __forceinline__ void diag_sincos(double v, double* s, double* c) {
  constexpr double kInv2PiHi = 0x1.45f306dc9c883p-3, kInv2PiLo = -0x1.6b01ec5417056p-57;
  const double k = rint(v * kInv2PiHi);
  const double r = fma(v, kInv2PiHi, -k) + v * kInv2PiLo;
  sincospi(2.0 * r, s, c);
}

// Steps 2 and 3 for the tile at `base`: E(base | (tid + it * kBlock)) into e[it].  W is zero on entry once every thread
// is past the barrier at the top (the last round of the previous tile zeroed it), and zero again on return.
__device__ __forceinline__ void diag_energies(const DiagArgs& a, u64 base, double* W, double* slots, double* e) {
  static_assert(kExpTileBits == 11 && kExpLoads == 8, "the rounds below are bits 0-2, 3-5, 6-7 and 8-10");
  const int tid = threadIdx.x;
  typedef __attribute__((address_space(4))) const DiagTerm cterm_t;
  typedef __attribute__((address_space(4))) const DiagPiece cpiece_t;
  typedef __attribute__((address_space(4))) const DiagJoin cjoin_t;
  cterm_t* const terms = (cterm_t*)(unsigned long long)a.terms;
  cpiece_t* const pieces = (cpiece_t*)(unsigned long long)a.pieces;
  cjoin_t* const joins = (cjoin_t*)(unsigned long long)a.joins;
  __syncthreads();                                  // W is zero: every thread is past the last round of the previous tile
  for (int p = tid; p < a.n_pieces; p += kBlock) {
    const int first = pieces[p].first, count = pieces[p].count, slot = pieces[p].slot;
    const unsigned zi = pieces[p].zi;
    double v = 0.0;
    for (int i = 0; i < count; ++i) {
      const double c = terms[first + i].c;
      v += (__popcll(base & terms[first + i].zo) & 1) ? -c : c;
    }
    if (slot < 0) W[zi] = v;
    else slots[slot] = v;
  }
  if (a.n_joins) {                                  // (the same in every thread)
    __syncthreads();
    for (int q = tid; q < a.n_joins; q += kBlock) {
      const int slot = joins[q].slot, count = joins[q].count;
      double v = slots[slot];
      for (int i = 1; i < count; ++i) v += slots[slot + i];
      W[joins[q].zi] = v;
    }
  }
  __syncthreads();
  diag_round<0, 3>(W);
  __syncthreads();
  diag_round<3, 3>(W);
  __syncthreads();
  diag_round<6, 2>(W);
  __syncthreads();
#pragma unroll
  for (int it = 0; it < kExpLoads; ++it) {          // bits 8-10: the thread's own slots, read by nobody else
    e[it] = W[tid + it * kBlock];
    W[tid + it * kBlock] = 0.0;
  }
  diag_butterflies<3>(e);
}

// step 1: the thread's slots of the tile at `base` (zero above the 2^tb amplitudes of a chunk smaller than a tile)
template <bool NT>
__device__ __forceinline__ void diag_load(const double2* amp, u64 base, int S, double2* x) {
#pragma unroll
  for (int it = 0; it < kExpLoads; ++it)
    x[it] = (int)threadIdx.x + it * kBlock < S ? ld_amp<NT>(amp + (base | (u64)((int)threadIdx.x + it * kBlock))) : make_double2(0.0, 0.0);
}

// Steps 1 to 3 for the workgroup's tiles o = blockIdx.x, blockIdx.x + gridDim.x, ..., then body(base, x, e) with the
// thread's amplitudes x[it] of a.amp and E in e[it], slot j = tid + it * kBlock (x is zero above S = 2^tb); body is a
// lambda marked always_inline.  The one place that owns W and the slots, and so the rule that W is zero on entry of
// diag_energies and on its return.
template <bool NT, class Body>
__device__ __forceinline__ void diag_tiles(const DiagArgs& a, Body body) {
  __shared__ double W[kExpTile];
  __shared__ double slots[kDiagMaxSlots];
#pragma unroll
  for (int it = 0; it < kExpLoads; ++it) W[(int)threadIdx.x + it * kBlock] = 0.0;
  for (u64 o = blockIdx.x; o < a.n_tiles; o += gridDim.x) {
    const u64 base = o << a.tb;
    double2 x[kExpLoads];
    diag_load<NT>(a.amp, base, 1 << a.tb, x);
    double e[kExpLoads];
    diag_energies(a, base, W, slots, e);
    body(base, x, e);
  }
}

// N running sums of the workgroup's threads into row[0 .. N-1]: lane tree, lane 0 of each wave into red[wave][i], then
// thread i adds red[0][i], red[1][i], ... in wave order, starting from red[0][i].  Every thread of the workgroup calls it.
template <int N>
__device__ __forceinline__ void block_sum_row(const double (&s)[N], double* row) {
  __shared__ double red[kBlock / 64][N];
  const int tid = threadIdx.x;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const double v = wave_sum(s[i]);
    if ((tid & 63) == 0) red[tid >> 6][i] = v;
  }
  __syncthreads();
  if (tid < N) {
    double v = red[0][tid];
    for (int w = 1; w < kBlock / 64; ++w) v += red[w][tid];
    row[tid] = v;
  }
}

template <bool NT, int MODE>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(4))) void k_diag_tile(const DiagArgs a) {
  const int S = 1 << a.tb;
  const int tid = threadIdx.x;
  if (MODE == kDiagPhase) {
    diag_tiles<NT>(a, [&](u64 base, const double2* x, const double* e) __attribute__((always_inline)) {
#pragma unroll
      for (int it = 0; it < kExpLoads; ++it) {
        double s, c;
        diag_sincos(a.gamma * e[it], &s, &c);
        if (tid + it * kBlock < S)
          st_amp<NT>(a.amp + (base | (u64)(tid + it * kBlock)),
                     make_double2(fma(x[it].x, c, x[it].y * s), fma(x[it].y, c, -(x[it].x * s))));
        __builtin_amdgcn_sched_barrier(0);          // one slot at a time: interleaved they need more than 128 VGPRs
      }
    });
  } else {
    double m[3] = {0.0, 0.0, 0.0};
    diag_tiles<NT>(a, [&](u64 base, const double2* x, const double* e) __attribute__((always_inline)) {
#pragma unroll
      for (int it = 0; it < kExpLoads; ++it) {
        const double p = fma(x[it].x, x[it].x, x[it].y * x[it].y), pe = p * e[it];
        m[0] += p;
        m[1] += pe;
        m[2] = fma(pe, e[it], m[2]);
      }
    });
    block_sum_row(m, a.partial + (u64)blockIdx.x * 3);
  }
}

// The values of the single terms, out[t] = sum_i |psi_i|^2 (-1)^popcount(i & z_t) (qsim_expectation_z_terms): the
// transpose of k_diag_tile.  There the terms are scattered into a spectrum and the transform gives E over the tile; here
// the tile's probabilities p_j = |psi_j|^2 are transformed and every term GATHERS its value at zi, with the outer sign
// (-1)^popcount(base & zo) (diag_plan.h).  Per tile: the thread's kExpLoads amplitudes -> p in registers, bits 8-10 of
// the transform on the thread's own slots tid + r * kBlock, p into the 16 KiB LDS array, bits 0-2, 3-5, 6-7 through LDS
// (the stages commute, so the register round comes first here), then one LDS read and one __popcll per term of the
// thread.  A pass serves at most kDiagValuesPerPass terms: term i of the pass belongs to thread i % kBlock, slot
// i / kBlock, whose (zi, zo) and running sum stay in registers over the workgroup's tiles; at the end the sums go
// straight into the workgroup's row of a.partial ([workgroup][a.n_terms]) -- no reduction inside the workgroup -- and
// k_hist_sum adds the rows in its fixed order.  No atomics; the state is only read.  Slots above 2^tb are zero
// (diag_load) and zi < 2^tb, so a chunk smaller than a tile needs no other code.
// Compiler's resource usage (gfx950, both NT forms alike): 96 VGPRs, 72 SGPRs, no spill, no scratch, 16 KiB of LDS: four
// workgroups per CU as asked for (amdgpu_waves_per_eu), like the siblings.
constexpr int kDiagValueSlots = kDiagValuesPerPass / kBlock;
static_assert(kDiagValuesPerPass % kBlock == 0, "a pass's terms are dealt to the threads in whole slots");

struct DiagValueArgs {
  const double2* amp;
  const DiagValueTerm* terms;   // the pass's records
  double* partial;              // [workgroup][n_terms]
  u64 n_tiles;                  // 2^(k - tb)
  int tb;                       // tile bits: min(k, kExpTileBits)
  int n_terms;                  // terms of this pass, 1 .. kDiagValuesPerPass
};

template <bool NT>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(4))) void k_diag_term_values(const DiagValueArgs a) {
  static_assert(kExpTileBits == 11 && kExpLoads == 8, "the rounds below are bits 8-10, 0-2, 3-5 and 6-7");
  __shared__ double P[kExpTile];
  const int S = 1 << a.tb;
  const int tid = threadIdx.x;
  const int n_slots = (a.n_terms + kBlock - 1) / kBlock;   // (the same in every thread)
  unsigned zi[kDiagValueSlots];
  u64 zo[kDiagValueSlots];
  double acc[kDiagValueSlots];
#pragma unroll
  for (int s = 0; s < kDiagValueSlots; ++s) {
    const int t = tid + s * kBlock;
    const bool mine = t < a.n_terms;                 // (a thread without a term in a slot gathers P[0]; nothing is written)
    zi[s] = mine ? a.terms[t].zi : 0u;
    zo[s] = mine ? a.terms[t].zo : 0ull;
    acc[s] = 0.0;
  }
  for (u64 o = blockIdx.x; o < a.n_tiles; o += gridDim.x) {
    const u64 base = o << a.tb;
    double p[kExpLoads];
    {
      double2 x[kExpLoads];
      diag_load<NT>(a.amp, base, S, x);
#pragma unroll
      for (int it = 0; it < kExpLoads; ++it) p[it] = fma(x[it].x, x[it].x, x[it].y * x[it].y);
    }
    diag_butterflies<3>(p);                          // bits 8-10
    __syncthreads();                                 // the gathers of the previous tile are done
#pragma unroll
    for (int it = 0; it < kExpLoads; ++it) P[tid + it * kBlock] = p[it];
    __syncthreads();
    diag_round<0, 3>(P);
    __syncthreads();
    diag_round<3, 3>(P);
    __syncthreads();
    diag_round<6, 2>(P);
    __syncthreads();
#pragma unroll
    for (int s = 0; s < kDiagValueSlots; ++s)
      if (s < n_slots) {
        const double v = P[zi[s]];
        acc[s] += (__popcll(base & zo[s]) & 1) ? -v : v;
      }
  }
  double* const row = a.partial + (u64)blockIdx.x * (u64)a.n_terms;
#pragma unroll
  for (int s = 0; s < kDiagValueSlots; ++s)
    if (tid + s * kBlock < a.n_terms) row[tid + s * kBlock] = acc[s];
}

// dst_j = E_j src_j (ACC false) or dst_j += E_j src_j (ACC true) over contiguous tiles; a.amp = src, a.other = dst.  dst
// may be src when writing: slot j is read and written by the same thread.  Compiler's resource usage (gfx950, both NT
// forms alike): writing 98 VGPRs, accumulating 128, overlap 112; no spill, no scratch, four workgroups per CU each.
template <bool NT, bool ACC>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(4))) void k_diag_apply(const DiagArgs a) {
  const int S = 1 << a.tb;
  const int tid = threadIdx.x;
  diag_tiles<NT>(a, [&](u64 base, const double2* x, const double* e) __attribute__((always_inline)) {
    double2 y[kExpLoads];
    if (ACC) diag_load<NT>(a.other, base, S, y);
#pragma unroll
    for (int it = 0; it < kExpLoads; ++it) {
      if (tid + it * kBlock >= S) continue;
      const double2 v = ACC ? make_double2(fma(e[it], x[it].x, y[it].x), fma(e[it], x[it].y, y[it].y))
                            : make_double2(e[it] * x[it].x, e[it] * x[it].y);
      st_amp<NT>(a.other + (base | (u64)(tid + it * kBlock)), v);
    }
  });
}

// sum_j conj(bra_j) ket_j and sum_j conj(bra_j) E_j ket_j, (re, im) each: a.amp = ket, a.other = bra (it may be ket);
// the workgroup's row of 4 partials into a.partial, by the reduction of the moments.
template <bool NT>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(4))) void k_diag_overlap(const DiagArgs a) {
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  diag_tiles<NT>(a, [&](u64 base, const double2* x, const double* e) __attribute__((always_inline)) {
    double2 b[kExpLoads];
    diag_load<NT>(a.other, base, 1 << a.tb, b);
#pragma unroll
    for (int it = 0; it < kExpLoads; ++it) {        // (slots above S hold zeros in x and b)
      const double re = fma(b[it].x, x[it].x, b[it].y * x[it].y), im = fma(b[it].x, x[it].y, -(b[it].y * x[it].x));
      s[0] += re;
      s[1] += im;
      s[2] = fma(re, e[it], s[2]);
      s[3] = fma(im, e[it], s[3]);
    }
  });
  block_sum_row(s, a.partial + (u64)blockIdx.x * 4);
}
