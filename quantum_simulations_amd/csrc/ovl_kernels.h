// ovl_kernels.h -- matrix elements of Pauli strings between two states: out[t] = <bra|P_t|ket> (qsim_overlap_pauli).
// Part of the single translation unit qsim_hip.hip (included there after psum_kernels.h; not a standalone header).
//
//   <bra|P|ket> = i^ny sum_j conj(bra_j) s(j ^ x) ket_{j ^ x},   s(i) = (-1)^popcount(i & z),
// complex; x = z = 0 gives <bra|ket>.  Masks, ny and s(i) as in pauli_tile.h; the passes are those of
// qsim_plan_expectation, and a term keeps g = i^ny in f0, f1 (kPauliSum without coefficients).
//
// Tile pass (k_ovl_tile): the tile walk of pauli_tile.h and the structure of k_expect_tile -- threads dealt out to
// (term, slice) pairs, running sums kept per thread across the tiles of the workgroup -- with TWO tiles in LDS, bra and
// ket, and two sums per term.  The sum runs over ALL j of the slice, not over the half space of k_expect_tile: that
// pairing rests on <psi|P|psi> being real, and the value here is complex.  i^ny and the outer sign are applied once per
// tile and term.  At the end the slices of a term are added in slice order into the workgroup's row of partials
// [workgroup][2 * n_terms], and k_hist_sum adds the rows in workgroup order: no atomics, every call gives the same bits.
// Two 11-bit tiles are 64 KiB of LDS: two workgroups per CU, so the grid is capped at kOvlMaxWg = 512.  (10-bit tiles
// would keep four, but the planner's 11-bit tile masks would no longer fit a tile.)  What the pass costs next to
// qsim_norm2 and qsim_expectation_pauli is measured in profiles/r18_hamiltonian_probe.json; the 10-bit form was not
// built, so the cost of the lower occupancy is known only as part of those figures.
//
// Wide pass (k_ovl_wide): one term whose x does not fit a tile; each lane reads bra_j and ket_{j ^ x}, one (re, im)
// partial per workgroup.  Correctness, not speed.
constexpr int kOvlMaxWg = 512;                      // workgroups per tile launch: 2 per CU at 64 KiB of LDS each

struct OvlArgs {
  const double2* bra;
  const double2* ket;
  const PauliTerm* terms;   // entries of kSumStride bytes
  double* partial;       // [workgroup][2 * n_terms]
  TileWalk w;
  int n_terms;           // <= kExpMaxTerms
  int slices;            // threads per term: a power of two, slices * min(n_terms, 256) <= 256
};

template <bool NT>
__global__ __launch_bounds__(kBlock) void k_ovl_tile(const OvlArgs a) {
  __shared__ double2 tile[2 * kExpTile];            // bra, then ket
  double2* const tb_ = tile;
  double2* const tk_ = tile + kExpTile;
  const int S = 1 << a.w.tb;
  const int tid = threadIdx.x;
  const int slice = tid & (a.slices - 1);
  const int per = kBlock / a.slices;                // terms per slot row
  u64 off[kExpLoads];
  tile_offsets(a.w, off);
  PauliTerm tm[kExpSlots];
  bool live[kExpSlots];
  double accr[kExpSlots], acci[kExpSlots];
#pragma unroll
  for (int s = 0; s < kExpSlots; ++s) {
    const int t = tid / a.slices + per * s;
    live[s] = t < a.n_terms;
    if (live[s]) term_load<kSumStride>(a.terms, t, &tm[s]);
    accr[s] = 0.0;
    acci[s] = 0.0;
  }
  for (u64 o = blockIdx.x; o < a.w.n_tiles; o += gridDim.x) {
    const u64 base = tile_base(a.w.outer_mask, o);
    double2 xb[kExpLoads], xk[kExpLoads];           // tile_load and tile_fill for both tiles at once, slot by slot
#pragma unroll
    for (int it = 0; it < kExpLoads; ++it)
      if (tid + it * kBlock < S) {
        xb[it] = ld_amp<NT>(a.bra + (base | off[it]));
        xk[it] = ld_amp<NT>(a.ket + (base | off[it]));
      }
    __syncthreads();                                // (the previous tiles are consumed)
#pragma unroll
    for (int it = 0; it < kExpLoads; ++it)
      if (tid + it * kBlock < S) {
        tb_[tid + it * kBlock] = xb[it];
        tk_[tid + it * kBlock] = xk[it];
      }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < kExpSlots; ++s) {
      if (!live[s]) continue;
      const PauliTerm& e = tm[s];
      double sr = 0.0, si = 0.0;                    // sum_j s(p) conj(bra_j) ket_p, p = j ^ xi
      for (int j = slice; j < S; j += a.slices) {
        const int p = j ^ (int)e.xi;
        const double2 u = tb_[j], w = tk_[p];
        const double re = fma(u.x, w.x, u.y * w.y), im = fma(u.x, w.y, -(u.y * w.x));
        if (__popc((unsigned)p & e.zi) & 1) { sr -= re; si -= im; } else { sr += re; si += im; }
      }
      const bool neg = __popcll(base & e.zo) & 1;   // the sign over the outer bits: one per tile and term
      const double vr = fma(e.f0, sr, -(e.f1 * si)), vi = fma(e.f0, si, e.f1 * sr);
      accr[s] += neg ? -vr : vr;
      acci[s] += neg ? -vi : vi;
    }
  }
  __syncthreads();
  double* red = reinterpret_cast<double*>(tile);    // [slot][re | im][thread]: 2 * kExpSlots * kBlock doubles (<= 4 kExpTile)
#pragma unroll
  for (int s = 0; s < kExpSlots; ++s) {
    red[(2 * s) * kBlock + tid] = accr[s];
    red[(2 * s + 1) * kBlock + tid] = acci[s];
  }
  __syncthreads();
  for (int t = tid; t < a.n_terms; t += kBlock) {   // term t: slot t / per, threads (t % per) * slices + 0 .. slices-1
    const double* r = red + (2 * (t / per)) * kBlock + (t % per) * a.slices;
    double vr = r[0], vi = r[kBlock];
    for (int sl = 1; sl < a.slices; ++sl) { vr += r[sl]; vi += r[kBlock + sl]; }
    a.partial[((u64)blockIdx.x * a.n_terms + t) * 2] = vr;
    a.partial[((u64)blockIdx.x * a.n_terms + t) * 2 + 1] = vi;
  }
}

struct OvlWideArgs {
  const double2* bra;
  const double2* ket;
  double* partial;       // [workgroup][2]
  u64 n;                 // amplitudes
  u64 x, z;
  double gr, gi;         // i^ny
};

template <bool NT>
__global__ __launch_bounds__(kBlock) void k_ovl_wide(const OvlWideArgs a) {
  __shared__ double part[2 * (kBlock / 64)];
  const u64 stride = (u64)gridDim.x * kBlock;
  double sr = 0.0, si = 0.0;
  for (u64 j = (u64)blockIdx.x * kBlock + threadIdx.x; j < a.n; j += stride) {
    const u64 p = j ^ a.x;
    const double2 u = ld_amp<NT>(a.bra + j), w = ld_amp<NT>(a.ket + p);
    const double re = fma(u.x, w.x, u.y * w.y), im = fma(u.x, w.y, -(u.y * w.x));
    if (__popcll(p & a.z) & 1) { sr -= re; si -= im; } else { sr += re; si += im; }
  }
  const double vr = wave_sum(fma(a.gr, sr, -(a.gi * si))), vi = wave_sum(fma(a.gr, si, a.gi * sr));
  if ((threadIdx.x & 63) == 0) { part[2 * (threadIdx.x >> 6)] = vr; part[2 * (threadIdx.x >> 6) + 1] = vi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double r = 0.0, im = 0.0;
    for (int w = 0; w < kBlock / 64; ++w) { r += part[2 * w]; im += part[2 * w + 1]; }
    a.partial[2 * blockIdx.x] = r;
    a.partial[2 * blockIdx.x + 1] = im;
  }
}
