// sample_kernels.h -- shot sampling of the full register (qsim_sample, qsim_sample_locate): a two-level inverse CDF.
// Part of the single translation unit qsim_hip.hip (included there, in order; not a standalone header).
//
// The chunk is cut into blocks of 2^kSampleBlockBits contiguous amplitudes (a chunk of fewer amplitudes is one block,
// padded with zeros).  Over the |amp|^2 of a block stands ONE summation tree, the balanced binary tree over contiguous
// index ranges: node(l, j) = node(l-1, 2j) + node(l-1, 2j+1), leaves node(0, i) = sample_prob(amp_i).
//   k_sample_block_sums (pass A) writes the root of every block: S[b].  A wave loads 16 rows of 64 contiguous amplitudes
//     (16 B per lane, 1 KiB per instruction), folds them over its lanes (sample_fold: levels 1..6 of the tree), then
//     the 16 rows (levels 7..10), and the four waves give levels 11 and 12.
//   k_sample_resolve (pass B) builds the SAME tree of a hit block in LDS -- level 1 by the same sample_fold step, the
//     levels above it as a heap -- so its root is S[b] bit for bit, and walks every shot of the block down the tree.
// Both are read-only, use no atomics and add in a fixed order: two calls give the same bits.
constexpr int kSampleBlockBits = 12;
constexpr u64 kSampleBlock = 1ull << kSampleBlockBits;
constexpr u64 kSampleMaxShots = 1ull << 24;
static_assert(kSampleBlockBits == 12 && kBlock == 256, "four waves of 16 rows of 64 amplitudes make one block");

__device__ __forceinline__ double sample_prob(double2 v) { return fma(v.x, v.x, v.y * v.y); }

// The |amp|^2 of the 16 rows of this wave: v[j] = amplitude ((wave * 16 + j) * 64 + lane) of block b (0 past the chunk).
template <bool NT>
__device__ __forceinline__ void sample_load_rows(const double2* __restrict__ amp, u64 n, u64 b, double (&v)[16]) {
  const u64 first = (b << kSampleBlockBits) + ((u64)(threadIdx.x >> 6) << 10) + (threadIdx.x & 63);
  double2 x[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const u64 i = first + (u64)j * 64;
    x[j] = i < n ? ld_amp<NT>(amp + i) : make_double2(0.0, 0.0);
  }
  __builtin_amdgcn_sched_barrier(0);                // every load in flight before the first use (as in k_hist)
#pragma unroll
  for (int j = 0; j < 16; ++j) v[j] = sample_prob(x[j]);
}

// One level of the tree across lanes, halving the registers: before, v[0 .. 2 * COUNT) of a lane are values of 2 * COUNT
// rows; after, v[m] is the sum over the lanes {lane, lane ^ OFF} of row 2 m + (bit OFF of lane).  (Both lanes of a pair
// add the same two values of the row they keep; a + b = b + a in every bit.)
template <int OFF, int COUNT>
__device__ __forceinline__ void sample_fold(double (&v)[16]) {
  const bool up = (threadIdx.x & OFF) != 0;
#pragma unroll
  for (int m = 0; m < COUNT; ++m) {
    const double keep = up ? v[2 * m + 1] : v[2 * m];
    const double send = up ? v[2 * m] : v[2 * m + 1];
    v[m] = keep + __shfl_xor(send, OFF, 64);
  }
}

template <bool NT>
__global__ __launch_bounds__(kBlock) void k_sample_block_sums(const double2* __restrict__ amp, u64 n, u64 n_blocks,
                                                              double* __restrict__ sums) {
  __shared__ double part[kBlock / 64];
  // XCD-contiguous workgroup order (logical_block<true>) when the grid is whole octets
  const u64 b = (((u64)gridDim.x * gridDim.y) & 7) ? logical_block<false>() : logical_block<true>();
  if (b >= n_blocks) return;                        // (the whole workgroup: a 2-D grid may round up)
  double v[16];
  sample_load_rows<NT>(amp, n, b, v);
  sample_fold<1, 8>(v);                             // levels 1..4: 16 rows -> 1 register, row (lane & 15) over 16 lanes
  sample_fold<2, 4>(v);
  sample_fold<4, 2>(v);
  sample_fold<8, 1>(v);
  double r = v[0];
  r += __shfl_xor(r, 16, 64);                       // levels 5, 6: every lane holds the sum of row (lane & 15)
  r += __shfl_xor(r, 32, 64);
#pragma unroll
  for (int off = 1; off < 16; off <<= 1) r += __shfl_xor(r, off, 64);   // levels 7..10: the wave's 16 rows, pairwise
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = r;
  __syncthreads();
  if (threadIdx.x == 0) sums[b] = (part[0] + part[1]) + (part[2] + part[3]);
}

// One workgroup per hit block g: block hit_block[g], its shots slot[hit_first[g] .. hit_first[g + 1]).  A slot holds the
// shot's local threshold (the bits of a double, >= 0) on entry and the chunk index of the sampled amplitude on exit.
//
// The walk: at a node with children L, R a threshold t < L goes left, any other goes right with t - L.  That is the
// search for the smallest i whose inclusive prefix exceeds t, the prefix being the one this tree defines (the sum of the
// left siblings on the way down), so it is monotone by construction.  t < node holds on the way (t < L going left; going
// right it is tested), hence every subtree entered has weight and the leaf reached has |amp|^2 > 0.  Where rounding has
// pushed t to or past the end of a subtree (t >= node: at the root when the block's own sum is below the difference of
// the block prefix, or after t - L), the answer is the last leaf with weight of that subtree (`last`: right when R > 0).
template <bool NT>
__global__ __launch_bounds__(kBlock) void k_sample_resolve(const double2* __restrict__ amp, u64 n, u64 n_blocks,
                                                           const u64* __restrict__ hit_block,
                                                           const unsigned* __restrict__ hit_first, u64 n_hit,
                                                           u64* __restrict__ slot) {
  constexpr int kHalf = 1 << (kSampleBlockBits - 1);
  __shared__ double tree[2 * kHalf];                // heap: tree[1] the root, children of j at 2 j and 2 j + 1;
                                                    // level 1 (pairs of leaves) at [kHalf, 2 kHalf); tree[0] unused
  const u64 g = logical_block<false>();
  if (g >= n_hit) return;
  const u64 b = hit_block[g];
  if (b >= n_blocks) return;
  double v[16];
  sample_load_rows<NT>(amp, n, b, v);
  sample_fold<1, 8>(v);                             // level 1: v[m] = the pair (lane >> 1) of row 2 m + (lane & 1)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int m = 0; m < 8; ++m) tree[kHalf + (wave * 16 + 2 * m + (lane & 1)) * 32 + (lane >> 1)] = v[m];
  __syncthreads();
  for (int w = kHalf >> 1; w >= 1; w >>= 1) {       // levels 2..12
    for (int j = w + threadIdx.x; j < 2 * w; j += kBlock) tree[j] = tree[2 * j] + tree[2 * j + 1];
    __syncthreads();
  }
  const u64 base = b << kSampleBlockBits;
  const unsigned end = hit_first[g + 1];
  for (unsigned s = hit_first[g] + threadIdx.x; s < end; s += kBlock) {
    double t = __longlong_as_double((long long)slot[s]);
    bool last = !(t < tree[1]);
    int j = 1;
    while (j < kHalf) {
      const double L = tree[2 * j], R = tree[2 * j + 1];
      if (last) j = 2 * j + (R > 0.0 ? 1 : 0);
      else if (t < L) j = 2 * j;
      else { t -= L; j = 2 * j + 1; last = !(t < R); }
    }
    const u64 i0 = base + 2 * (u64)(j - kHalf);     // the two leaves of the pair, read again (the block was just loaded)
    const double p0 = i0 < n ? sample_prob(amp[i0]) : 0.0;
    const double p1 = i0 + 1 < n ? sample_prob(amp[i0 + 1]) : 0.0;
    const bool right = last ? p1 > 0.0 : !(t < p0);
    slot[s] = i0 + (right ? 1 : 0);
  }
}

// ---- the host part: block prefix -> per shot the block and the local threshold (pure functions)
static bool sample_randnum_ok(double r) { return r >= 0.0 && r < 1.0; }   // (NaN fails both; -0.0 passes)

// cdf[0 .. n_blocks): inclusive, non-decreasing, cdf[n_blocks - 1] = total > 0.  Block of r: the smallest b with
// cdf[b] > r * total (its weight cdf[b] - cdf[b - 1] is then > 0); r * total at or above cdf[last] (rounding): the last
// block with weight.  Local threshold: r * total - cdf[b - 1] >= 0.
static void sample_locate(u64 n_blocks, const double* cdf, u64 n_shots, const double* randnums, uint64_t* out_block, double* out_local) {
  const double total = cdf[n_blocks - 1];
  u64 last = n_blocks - 1;
  while (last > 0 && !(cdf[last] > cdf[last - 1])) --last;
  for (u64 s = 0; s < n_shots; ++s) {
    const double t = randnums[s] * total + 0.0;     // (+ 0.0: -0.0 becomes 0.0)
    u64 b = (u64)(std::upper_bound(cdf, cdf + n_blocks, t) - cdf);
    if (b >= n_blocks) b = last;
    out_block[s] = b;
    out_local[s] = b ? t - cdf[b - 1] : t;
  }
}
