// expect_kernels.h -- expectation values of Pauli sums (qsim_plan_expectation, qsim_expectation_pauli).
// Part of the single translation unit qsim_hip.hip (included there after pauli_tile.h; not a standalone header).
//
// Masks, ny and s(i) as in pauli_tile.h:   <psi|P|psi> = sum_i s(i) Re(i^ny conj(psi_{i ^ x}) psi_i).
// Pairing i with i ^ x (h = the top bit of x, i runs over the half with bit h clear) the two halves give the same real
// part, so for x != 0 the value is 2 sum_{i: bit h clear} s(i) Re(i^ny c_i), c_i = conj(psi_{i ^ x}) psi_i.
//
// Tile pass (k_expect_tile): the tile walk of pauli_tile.h, read-only; every term of the pass is evaluated from the tile
// in LDS.  A term keeps (cr, ci) in f0, f1: value = cr * sum s Re(c) + ci * sum s Im(c) (kPauliExpect: the factor
// i^ny, and 2 for pairs); the outer sign is one multiply per tile and term.  Threads are dealt out to (term, slice)
// pairs -- 256 / n_terms slices per term for few terms, a term per thread (up to four) for many -- and keep a running
// sum per term across their tiles, so nothing is reduced per tile.  At the end the slices of a term are added in slice
// order into the workgroup's row of partials, and k_hist_sum adds the rows in workgroup order: no atomics anywhere,
// every call gives the same bits.  The evaluation is a direct sum per term over the tile (2 LDS reads and a handful of
// FMAs per amplitude pair and term), so beyond about 4 terms the pass is bound by that sum, not by HBM
// (profiles/r07_expectation_probe.json).
//
// Wide-X pass (k_expect_wide): one term whose x does not fit a tile with the line bits; each lane loads psi_i and
// psi_{i ^ x} for i with bit h clear (every amplitude read once), one partial per workgroup.  Correctness, not speed.
struct ExpArgs {
  const double2* amp;
  const PauliTerm* terms;   // whole records
  double* partial;       // [workgroup][n_terms]
  TileWalk w;
  int n_terms;           // <= kExpMaxTerms
  int slices;            // threads per term: a power of two, slices * min(n_terms, 256) <= 256
};

template <bool NT>
__global__ __launch_bounds__(kBlock) void k_expect_tile(const ExpArgs a) {
  __shared__ double2 tile[kExpTile];
  const int S = 1 << a.w.tb;
  const int tid = threadIdx.x;
  const int slice = tid & (a.slices - 1);
  const int per = kBlock / a.slices;                // terms per slot row
  u64 off[kExpLoads];
  tile_offsets(a.w, off);
  PauliTerm tm[kExpSlots];
  bool live[kExpSlots];
  double acc[kExpSlots];
#pragma unroll
  for (int s = 0; s < kExpSlots; ++s) {
    const int t = tid / a.slices + per * s;
    live[s] = t < a.n_terms;
    if (live[s]) term_load<kTermStride>(a.terms, t, &tm[s]);
    acc[s] = 0.0;
  }
  for (u64 o = blockIdx.x; o < a.w.n_tiles; o += gridDim.x) {
    const u64 base = tile_base(a.w.outer_mask, o);
    double2 x[kExpLoads];
    tile_load<NT>(a.amp, base, off, S, x);
    __syncthreads();                                // (the previous tile is consumed)
    tile_fill(tile, S, x);
    __syncthreads();
#pragma unroll
    for (int s = 0; s < kExpSlots; ++s) {
      if (!live[s]) continue;
      const PauliTerm& e = tm[s];
      double sr = 0.0, si = 0.0;
      if (e.h < 0) {
        for (int j = slice; j < S; j += a.slices) {
          const double2 v = tile[j];
          const double p = fma(v.x, v.x, v.y * v.y);
          sr += (__popc((unsigned)j & e.zi) & 1) ? -p : p;
        }
      } else {
        const int low = (1 << e.h) - 1;
        for (int m = slice; m < (S >> 1); m += a.slices) {
          const int j = ((m & ~low) << 1) | (m & low);
          const double2 u = tile[j], w = tile[j ^ (int)e.xi];
          const double re = fma(w.x, u.x, w.y * u.y), im = fma(w.x, u.y, -(w.y * u.x));
          if (__popc((unsigned)j & e.zi) & 1) { sr -= re; si -= im; } else { sr += re; si += im; }
        }
      }
      const double v = fma(e.f0, sr, e.f1 * si);
      acc[s] += (__popcll(base & e.zo) & 1) ? -v : v;
    }
  }
  __syncthreads();
  double* red = reinterpret_cast<double*>(tile);    // [slot][thread]: kExpSlots * kBlock doubles (<= 2 kExpTile)
#pragma unroll
  for (int s = 0; s < kExpSlots; ++s) red[s * kBlock + tid] = acc[s];
  __syncthreads();
  for (int t = tid; t < a.n_terms; t += kBlock) {   // term t: slot t / per, threads (t % per) * slices + 0 .. slices-1
    const double* r = red + (t / per) * kBlock + (t % per) * a.slices;
    double v = r[0];
    for (int sl = 1; sl < a.slices; ++sl) v += r[sl];
    a.partial[(u64)blockIdx.x * a.n_terms + t] = v;
  }
}

struct ExpWideArgs {
  const double2* amp;
  double* partial;       // [workgroup]
  u64 half;              // amplitudes / 2
  u64 x, z;
  double cr, ci;
  int h;
};

template <bool NT>
__global__ __launch_bounds__(kBlock) void k_expect_wide(const ExpWideArgs a) {
  const u64 stride = (u64)gridDim.x * kBlock;
  const u64 low = (1ull << a.h) - 1;
  double sr = 0.0, si = 0.0;
  for (u64 m = (u64)blockIdx.x * kBlock + threadIdx.x; m < a.half; m += stride) {
    const u64 i = ((m & ~low) << 1) | (m & low);
    const double2 u = ld_amp<NT>(a.amp + i), w = ld_amp<NT>(a.amp + (i ^ a.x));
    const double re = fma(w.x, u.x, w.y * u.y), im = fma(w.x, u.y, -(w.y * u.x));
    if (__popcll(i & a.z) & 1) { sr -= re; si -= im; } else { sr += re; si += im; }
  }
  block_reduce_store<false>(fma(a.cr, sr, a.ci * si), a.partial);
}
