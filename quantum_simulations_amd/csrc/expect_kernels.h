// expect_kernels.h -- expectation values of Pauli sums (qsim_plan_expectation, qsim_expectation_pauli).
// Part of the single translation unit qsim_hip.hip (included there after readout_kernels.h; not a standalone header).
//
// A Pauli string is two masks of physical index bits: x = the bits that carry X or Y, z = the bits that carry Z or Y.
// With ny = popcount(x & z) (Y = i X Z):   <psi|P|psi> = sum_i (-1)^popcount(i & z) Re(i^ny conj(psi_{i ^ x}) psi_i).
// Pairing i with i ^ x (h = the top bit of x, i runs over the half with bit h clear) the two halves give the same real
// part, so for x != 0 the value is 2 sum_{i: bit h clear} s(i) Re(i^ny c_i), c_i = conj(psi_{i ^ x}) psi_i.
//
// Tile pass (k_expect_tile): a set T of tile bits (<= 11, the line bits 0..2 among them: every global access is a whole
// 128-byte line).  A workgroup walks tiles (the 2^|T| amplitudes with fixed outer bits), loads each into LDS with the
// loads of k_hist, and evaluates every term of the pass whose x lies in T from LDS.  The sign factors over tile and
// outer bits, s(i, z) = s(inner, z & T) s(outer, z & ~T): one multiply per tile and term.  Threads are dealt out to
// (term, slice) pairs -- 256 / n_terms slices per term for few terms, a term per thread (up to four) for many -- and
// keep a running sum per term across their tiles, so nothing is reduced per tile.  At the end the slices of a term are
// added in slice order into the workgroup's row of partials, and k_hist_sum adds the rows in workgroup order: no
// atomics anywhere, every call gives the same bits.  The evaluation is a direct sum per term over the tile (2 LDS reads
// and a handful of FMAs per amplitude pair and term), so beyond about 4 terms the pass is bound by that sum, not by HBM
// (profiles/r07_expectation_probe.json).
//
// Wide-X pass (k_expect_wide): one term whose x does not fit a tile with the line bits; each lane loads psi_i and
// psi_{i ^ x} for i with bit h clear (every amplitude read once), one partial per workgroup.  Correctness, not speed.
constexpr int kExpTileBits = 11;                    // the fused pass's tile width: 2^11 amplitudes = 32 KiB of LDS
constexpr int kExpMaxTerms = 1024;                  // terms per tile launch (the planner opens a new pass beyond)
constexpr int kExpSlots = kExpMaxTerms / kBlock;    // terms one thread evaluates at most
constexpr int kExpMaxWg = 1024;                     // workgroups per launch: 4 per CU at 32 KiB of LDS each
constexpr int kExpLineBits = 3;                     // 128-byte lines: 8 amplitudes

struct ExpTerm {         // one term of a tile pass in tile coordinates (inner bit b <-> physical bit tile_bit[b])
  u64 zo;                // z outside the tile (physical bits): the outer sign
  double cr, ci;         // value = cr * sum s Re(c) + ci * sum s Im(c)  (the factor i^ny, and 2 for pairs)
  unsigned xi, zi;       // x and z & T compressed onto the tile bits
  int h;                 // the top bit of xi (the loop runs over the half with it clear); -1: x = 0
  int pad_;
};

struct ExpArgs {
  const double2* amp;
  const ExpTerm* terms;
  double* partial;       // [workgroup][n_terms]
  u64 n_tiles;           // 2^(k - tb)
  u64 outer_mask;        // physical bits outside the tile (outer index bit j <-> the j-th set bit)
  int tile_bit[kExpTileBits];
  int tb;                // tile bits
  int n_terms;           // <= kExpMaxTerms
  int slices;            // threads per term: a power of two, slices * min(n_terms, 256) <= 256
};

template <bool NT>
__global__ __launch_bounds__(kBlock) void k_expect_tile(const ExpArgs a) {
  constexpr int kTile = 1 << kExpTileBits;
  constexpr int kLoads = kTile / kBlock;
  __shared__ double2 tile[kTile];
  const int S = 1 << a.tb;
  const int tid = threadIdx.x;
  const int slice = tid & (a.slices - 1);
  const int per = kBlock / a.slices;                // terms per slot row
  u64 off[kLoads];                                  // physical offsets of the amplitudes this thread loads (every tile)
#pragma unroll
  for (int it = 0; it < kLoads; ++it) {
    const int j = tid + it * kBlock;
    u64 o = 0;
    for (int b = 0; b < a.tb; ++b) o |= (u64)((j >> b) & 1) << a.tile_bit[b];
    off[it] = o;
  }
  ExpTerm tm[kExpSlots];
  bool live[kExpSlots];
  double acc[kExpSlots];
#pragma unroll
  for (int s = 0; s < kExpSlots; ++s) {
    const int t = tid / a.slices + per * s;
    live[s] = t < a.n_terms;
    if (live[s]) tm[s] = a.terms[t];
    acc[s] = 0.0;
  }
  for (u64 o = blockIdx.x; o < a.n_tiles; o += gridDim.x) {
    u64 base = 0;                                   // the outer index o deposited on the outer bits
    {
      u64 m = a.outer_mask, v = o;
      while (m) {
        const u64 low = m & (~m + 1);
        if (v & 1) base |= low;
        v >>= 1;
        m ^= low;
      }
    }
    double2 x[kLoads];
#pragma unroll
    for (int it = 0; it < kLoads; ++it)
      if (tid + it * kBlock < S) x[it] = ld_amp<NT>(a.amp + (base | off[it]));
    __syncthreads();                                // (the previous tile is consumed)
#pragma unroll
    for (int it = 0; it < kLoads; ++it)
      if (tid + it * kBlock < S) tile[tid + it * kBlock] = x[it];
    __syncthreads();
#pragma unroll
    for (int s = 0; s < kExpSlots; ++s) {
      if (!live[s]) continue;
      const ExpTerm& e = tm[s];
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
      const double v = fma(e.cr, sr, e.ci * si);
      acc[s] += (__popcll(base & e.zo) & 1) ? -v : v;
    }
  }
  __syncthreads();
  double* red = reinterpret_cast<double*>(tile);    // [slot][thread]: kExpSlots * kBlock doubles (<= 2 kTile)
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

// ---- host: the pass plan (pure, no GPU)
// Greedy and deterministic: terms with x != 0 in input order go into the first pass whose tile bits (the union of its
// terms' x and the line bits) stay within kExpTileBits with the term added and that holds fewer than kExpMaxTerms
// terms, else into a new pass; a term whose x does not fit any tile gets a wide-X pass of its own.  Terms with x = 0
// then fill the tile passes in order (a new pass when none has room).  Each tile pass's bits are completed to
// min(k, kExpTileBits) with the lowest free bits.  Passes: the tile passes in creation order, then the wide-X passes in
// term order (tile mask 0).
struct ExpPlan {
  std::vector<int32_t> pass_of;   // per term
  std::vector<u64> tile;          // per pass (0: wide-X)
  std::vector<int> count;         // terms per pass
};

static int plan_expectation(int k, int n_terms, const uint64_t* x, ExpPlan* p) {
  if (k < 0 || k > 63) return fail(QSIM_ERR_INVALID, "qsim_plan_expectation: %d local qubits", k);
  if (n_terms < 0) return fail(QSIM_ERR_INVALID, "qsim_plan_expectation: n_terms = %d", n_terms);
  if (n_terms > 0 && !x) return fail(QSIM_ERR_INVALID, "qsim_plan_expectation: null x_masks");
  const u64 all = k >= 64 ? ~0ull : ((1ull << k) - 1);
  for (int t = 0; t < n_terms; ++t)
    if (x[t] & ~all)
      return fail(QSIM_ERR_NONLOCAL, "term %d: X/Y on index bit %d >= log2(chunk_size)=%d", t, 63 - __builtin_clzll(x[t] & ~all), k);
  const int K = std::min(k, kExpTileBits);
  const u64 line = (1ull << std::min(k, kExpLineBits)) - 1;
  p->pass_of.assign((size_t)n_terms, -1);
  p->tile.clear();
  p->count.clear();
  std::vector<int> wide;
  for (int t = 0; t < n_terms; ++t) {
    if (!x[t]) continue;
    if (__builtin_popcountll(x[t] | line) > K) { wide.push_back(t); continue; }
    size_t q = 0;
    while (q < p->tile.size() && (p->count[q] >= kExpMaxTerms || __builtin_popcountll(p->tile[q] | x[t]) > K)) ++q;
    if (q == p->tile.size()) { p->tile.push_back(line); p->count.push_back(0); }
    p->tile[q] |= x[t];
    ++p->count[q];
    p->pass_of[(size_t)t] = (int32_t)q;
  }
  for (int t = 0; t < n_terms; ++t) {
    if (x[t]) continue;
    size_t q = 0;
    while (q < p->tile.size() && p->count[q] >= kExpMaxTerms) ++q;
    if (q == p->tile.size()) { p->tile.push_back(line); p->count.push_back(0); }
    ++p->count[q];
    p->pass_of[(size_t)t] = (int32_t)q;
  }
  for (u64& m : p->tile)
    for (int b = 0; b < k && __builtin_popcountll(m) < K; ++b) m |= 1ull << b;
  for (int t : wide) {
    p->pass_of[(size_t)t] = (int32_t)p->tile.size();
    p->tile.push_back(0);
    p->count.push_back(1);
  }
  return QSIM_OK;
}

// (cr, ci) of a term: Re(i^ny c) = re, -im, -re, im for ny = 0..3; twice that for x != 0 (the pairs i, i ^ x)
static void exp_phase(u64 x, u64 z, double* cr, double* ci) {
  static const double kr[4] = {1.0, 0.0, -1.0, 0.0}, ki[4] = {0.0, -1.0, 0.0, 1.0};
  const int ny = __builtin_popcountll(x & z) & 3;
  const double f = x ? 2.0 : 1.0;
  *cr = f * kr[ny];
  *ci = f * ki[ny];
}

static u64 exp_pext(u64 v, u64 mask) {
  u64 r = 0;
  for (int j = 0; mask; mask &= mask - 1, ++j)
    if (v & mask & (~mask + 1)) r |= 1ull << j;
  return r;
}
