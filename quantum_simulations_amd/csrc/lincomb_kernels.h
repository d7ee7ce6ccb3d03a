// lincomb_kernels.h -- k_lincomb: a linear combination of up to five states with the inner products and the norm of the
// result taken in the same pass (qsim_lincomb, abi_lincomb.h).
// Part of the single translation unit qsim_hip.hip (included there, in order; not a standalone header).
//
// A block is kBlock * kLcItems consecutive amplitudes (16 KiB of every stream); a wave instruction covers 1 KiB, 16 B per
// lane.  A call that reduces something runs on a grid bounded by kLcMaxWg, so the per-workgroup partial rows are:
// workgroup w walks the blocks w, w + G, w + 2G, ... in ascending order (all workgroups advance as one front through
// every stream), with the XCD-contiguous workgroup order of k_hist where the grid is whole octets.  A call that only
// writes has no rows to bound and gets one workgroup per block, the shape of k_copy.  A thread keeps ONE running sum per reduced value over its
// items and blocks, in that order; the workgroup's sums go lane tree -> waves in wave order -> its partial row, and
// k_hist_sum adds the rows in row order.  No atomics anywhere: every run gives the same bits.
//
// Streams: dst (read iff RD, written iff WR), NSRC sources and NB bras that are not one of the sources.  A bra that IS a
// source costs no load: the source's registers are reduced against the new dst (`src_dot`).  The host maps the kernel's
// value slots (source s: 2s, 2s + 1; bra j: 2 NSRC + 2j, + 1; the norm last) to the columns of the partial row.
constexpr int kLcItems = 4;
constexpr unsigned kLcMaxWg = 2048;
constexpr int kLcMaxStreams = 4;                    // sources, and bras, of one call
constexpr int kLcMaxWidth = 2 * kLcMaxStreams + 1;  // reduced doubles of one call: (re, im) per bra and the norm
constexpr int kLcSlots = 4 * kLcMaxStreams + 1;     // value slots of the kernel (sources, own bras, norm)

struct LincombArgs {
  double2* dst;
  const double2* src[kLcMaxStreams];
  const double2* bra[kLcMaxStreams];
  double2 cd;                      // dst's coefficient (RD only)
  double2 cs[kLcMaxStreams];
  u64 n;                           // amplitudes (threads past n load and store nothing: chunks of fewer than 1024)
  u64 blocks;
  double* partial;                 // [workgroup][width]
  int width;                       // 0: nothing is reduced
  int src_dot;                     // bit s: <src_s|dst> is wanted
  int want_norm;
  signed char slot_of_col[kLcMaxWidth];
};

template <bool NT, bool RD, bool WR, int NSRC, int NB, int ITEMS = kLcItems>
__global__ __launch_bounds__(kBlock) void k_lincomb(const LincombArgs a) {
  static_assert(WR || (RD && NSRC == 0), "the read-only form has no sources");
  constexpr int NS1 = NSRC ? NSRC : 1, NB1 = NB ? NB : 1;
  const u64 wg = (gridDim.x & 7) ? (u64)blockIdx.x : logical_block<true>();
  double sr[NS1], si[NS1], br[NB1], bi[NB1], nrm = 0.0;
#pragma unroll
  for (int s = 0; s < NS1; ++s) sr[s] = si[s] = 0.0;
#pragma unroll
  for (int j = 0; j < NB1; ++j) br[j] = bi[j] = 0.0;
  for (u64 blk = wg; blk < a.blocks; blk += gridDim.x) {
    const u64 first = blk * (u64)(kBlock * ITEMS) + threadIdx.x;
    double2 d[ITEMS], x[NS1][ITEMS], y[NB1][ITEMS];
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
      const u64 i = first + (u64)it * kBlock;
      const bool in = i < a.n;
      d[it] = make_double2(0.0, 0.0);
      if (RD && in) d[it] = ld_amp<NT>(a.dst + i);
#pragma unroll
      for (int s = 0; s < NSRC; ++s) x[s][it] = in ? ld_amp<NT>(a.src[s] + i) : make_double2(0.0, 0.0);
#pragma unroll
      for (int j = 0; j < NB; ++j) y[j][it] = in ? ld_amp<NT>(a.bra[j] + i) : make_double2(0.0, 0.0);
    }
    __builtin_amdgcn_sched_barrier(0);              // every load of the block in flight before the first use
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
      const u64 i = first + (u64)it * kBlock;
      double2 v = d[it];
      if (WR) {
        if (RD) v = cmul(a.cd, v);                  // a_d dst first, then the sources in list order
#pragma unroll
        for (int s = 0; s < NSRC; ++s) v = cfma(a.cs[s], x[s][it], v);
        if (i < a.n) st_amp<NT>(a.dst + i, v);
      }
#pragma unroll
      for (int s = 0; s < NSRC; ++s)
        if ((a.src_dot >> s) & 1) {                 // conj(src) * v
          sr[s] = fma(x[s][it].x, v.x, fma(x[s][it].y, v.y, sr[s]));
          si[s] = fma(x[s][it].x, v.y, fma(-x[s][it].y, v.x, si[s]));
        }
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        br[j] = fma(y[j][it].x, v.x, fma(y[j][it].y, v.y, br[j]));
        bi[j] = fma(y[j][it].x, v.y, fma(-y[j][it].y, v.x, bi[j]));
      }
      if (a.want_norm) nrm = fma(v.x, v.x, fma(v.y, v.y, nrm));
    }
  }
  if (a.width == 0) return;
  __shared__ double part[kBlock / 64][kLcSlots];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int s = 0; s < NSRC; ++s) {
    const double r = wave_sum(sr[s]), m = wave_sum(si[s]);
    if (lane == 0) { part[wave][2 * s] = r; part[wave][2 * s + 1] = m; }
  }
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    const double r = wave_sum(br[j]), m = wave_sum(bi[j]);
    if (lane == 0) { part[wave][2 * NSRC + 2 * j] = r; part[wave][2 * NSRC + 2 * j + 1] = m; }
  }
  nrm = wave_sum(nrm);
  if (lane == 0) part[wave][kLcSlots - 1] = nrm;
  __syncthreads();
  if ((int)threadIdx.x < a.width) {
    const int slot = a.slot_of_col[threadIdx.x];
    double s = part[0][slot];
    for (int w = 1; w < kBlock / 64; ++w) s += part[w][slot];
    a.partial[wg * (u64)a.width + threadIdx.x] = s;
  }
}

// The instantiation for (rd, wr, n_src, n_bra) at run time.  The read-only form (rd && !wr) has no sources.
template <bool NT, bool RD, bool WR, int NSRC, int ITEMS>
static void launch_lincomb_nb(int nb, unsigned grid, hipStream_t stream, const LincombArgs& a) {
  switch (nb) {
    case 0: hipLaunchKernelGGL((k_lincomb<NT, RD, WR, NSRC, 0, ITEMS>), dim3(grid), dim3(kBlock), 0, stream, a); break;
    case 1: hipLaunchKernelGGL((k_lincomb<NT, RD, WR, NSRC, 1, ITEMS>), dim3(grid), dim3(kBlock), 0, stream, a); break;
    case 2: hipLaunchKernelGGL((k_lincomb<NT, RD, WR, NSRC, 2, ITEMS>), dim3(grid), dim3(kBlock), 0, stream, a); break;
    case 3: hipLaunchKernelGGL((k_lincomb<NT, RD, WR, NSRC, 3, ITEMS>), dim3(grid), dim3(kBlock), 0, stream, a); break;
    default: hipLaunchKernelGGL((k_lincomb<NT, RD, WR, NSRC, 4, ITEMS>), dim3(grid), dim3(kBlock), 0, stream, a); break;
  }
}
template <bool NT, bool RD, int ITEMS>
static void launch_lincomb_write(int nsrc, int nb, unsigned grid, hipStream_t stream, const LincombArgs& a) {
  switch (nsrc) {
    case 0: launch_lincomb_nb<NT, RD, true, 0, ITEMS>(nb, grid, stream, a); break;
    case 1: launch_lincomb_nb<NT, RD, true, 1, ITEMS>(nb, grid, stream, a); break;
    case 2: launch_lincomb_nb<NT, RD, true, 2, ITEMS>(nb, grid, stream, a); break;
    case 3: launch_lincomb_nb<NT, RD, true, 3, ITEMS>(nb, grid, stream, a); break;
    default: launch_lincomb_nb<NT, RD, true, 4, ITEMS>(nb, grid, stream, a); break;
  }
}
template <bool NT, int ITEMS = kLcItems>
static void launch_lincomb(bool rd, bool wr, int nsrc, int nb, unsigned grid, hipStream_t stream, const LincombArgs& a) {
  if (!wr) launch_lincomb_nb<NT, true, false, 0, ITEMS>(nb, grid, stream, a);
  else if (rd) launch_lincomb_write<NT, true, ITEMS>(nsrc, nb, grid, stream, a);
  else launch_lincomb_write<NT, false, ITEMS>(nsrc, nb, grid, stream, a);
}
