// readout_kernels.h -- what every read-only pass over a chunk shares: the block reductions, the norm, the histogram and
// its row sum, the sparse export, the closed-form checker, the fingerprint, the chunk's device buffers and the finish of
// a call.
// Part of the single translation unit qsim_hip.hip (included there, in order; not a standalone header).
constexpr int kReduceBlocks = 2048;

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
// The maximum that keeps a NaN: fmax and std::max drop a NaN operand, and a checker built on them calls a chunk of NaNs
// exact.  Once r is NaN no comparison is true any more, so it stays.
__host__ __device__ __forceinline__ double max_keep_nan(double r, double v) { return (v > r || v != v) ? v : r; }
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = max_keep_nan(v, __shfl_xor(v, off, 64));
  return v;
}

template <bool MAX>
__device__ __forceinline__ void block_reduce_store(double v, double* out) {
  __shared__ double part[kBlock / 64];
  v = MAX ? wave_max(v) : wave_sum(v);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    double r = part[0];
    for (int w = 1; w < kBlock / 64; ++w) r = MAX ? max_keep_nan(r, part[w]) : r + part[w];
    out[blockIdx.x] = r;
  }
}

__global__ __launch_bounds__(kBlock) void k_norm2_partial(const double2* p, u64 n, double* partial) {
  const u64 stride = (u64)gridDim.x * blockDim.x;
  double acc = 0.0;
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const double2 v = p[i];
    acc = fma(v.x, v.x, fma(v.y, v.y, acc));
  }
  block_reduce_store<false>(acc, partial);
}

// ---- joint outcome probabilities of r <= 8 qubits (qsim_probabilities): one read-only pass, a fixed summation order.
// Index bits 0..7 are the 256 threads of a workgroup (a wave reads 1 KiB contiguous, 16 B per lane).  The host deals the
// bits above out as ITEM bits (<= 3: the 2^ITEM amplitudes a thread loads per step), WORKGROUP bits (<= 11) and LOOP bits
// (walked in ascending order by every workgroup).  Selected qubits above bit 7 go to item and workgroup bits first -- at
// most 8 of them against up to 14 places -- so the bin of an amplitude depends on its lane, item and workgroup, never on
// the loop step, and a thread keeps one running sum per item.  At the end each wave folds its lanes over the lane bits
// that are NOT selected (butterfly; lanes a and a ^ off add the same two values), one lane per bin adds the result into
// the wave's row of an LDS histogram, and the four rows go in wave order into the workgroup's partial histogram.
// k_hist_sum adds the partials in workgroup order.  No atomics anywhere: every run gives the same bits.
struct HistArgs {
  const double2* amp;
  u64 n;                  // amplitudes (threads >= n load nothing: chunks of fewer than 256)
  u64 loop_mask;          // index bits walked by the loop (none of them selected)
  int item_bit[3];        // index bit of item bit j
  int wg_bit[11];         // index bit of workgroup-id bit j
  int n_wg_bits;
  int q[8];               // bin bit j <-> index bit q[j]
  int r;
  int lane_sel;           // the selected index bits among bits 0..5 (inside a wave), as a mask
  double* partial;        // [workgroup][2^r]
};
template <int ITEM_BITS, bool NT>
__global__ __launch_bounds__(kBlock) void k_hist(const HistArgs a) {
  constexpr int ITEMS = 1 << ITEM_BITS;
  __shared__ double hist[(kBlock / 64) * 256];
  const int nbins = 1 << a.r;
  // XCD-contiguous workgroup order (logical_block<true>) when the grid is whole octets
  const u64 wg = (gridDim.x & 7) ? (u64)blockIdx.x : logical_block<true>();
  for (int i = threadIdx.x; i < (kBlock / 64) * nbins; i += kBlock) hist[i] = 0.0;
  u64 base = threadIdx.x;
  for (int j = 0; j < a.n_wg_bits; ++j) base |= ((wg >> j) & 1ull) << a.wg_bit[j];
  u64 item_off[ITEMS];
#pragma unroll
  for (int it = 0; it < ITEMS; ++it) {
    u64 o = 0;
#pragma unroll
    for (int j = 0; j < ITEM_BITS; ++j) o |= (u64)((it >> j) & 1) << a.item_bit[j];
    item_off[it] = o;
  }
  double acc[ITEMS];
#pragma unroll
  for (int it = 0; it < ITEMS; ++it) acc[it] = 0.0;
  if (base < a.n) {
    u64 t = 0;                                      // the loop bits' values in ascending order (subset enumeration)
    do {
      double2 x[ITEMS];
#pragma unroll
      for (int it = 0; it < ITEMS; ++it) x[it] = ld_amp<NT>(a.amp + (base | item_off[it] | t));
      __builtin_amdgcn_sched_barrier(0);            // every load of the step in flight before the first use (hipcc interleaves
                                                    // them with the sums otherwise: two 16-B loads in flight per lane)
#pragma unroll
      for (int it = 0; it < ITEMS; ++it) acc[it] = fma(x[it].x, x[it].x, fma(x[it].y, x[it].y, acc[it]));
      t = ((t | ~a.loop_mask) + 1) & a.loop_mask;
    } while (t);
  }
  __syncthreads();                                  // (the histogram rows are zeroed)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int it = 0; it < ITEMS; ++it) {
    double v = acc[it];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
      if (!(a.lane_sel & off)) v += __shfl_xor(v, off, 64);
    if ((lane & ~a.lane_sel) == 0) {
      const u64 i0 = base | item_off[it];
      int m = 0;
      for (int j = 0; j < a.r; ++j) m |= (int)((i0 >> a.q[j]) & 1) << j;
      hist[wave * nbins + m] += v;
    }
  }
  __syncthreads();
  for (int m = threadIdx.x; m < nbins; m += kBlock) {
    double s = hist[m];
    for (int w = 1; w < kBlock / 64; ++w) s += hist[w * nbins + m];
    a.partial[wg * (u64)nbins + m] = s;
  }
}

// bin blockIdx.x of the partial histograms of n_wg workgroups: strided per thread, then the block reduction (fixed order)
__global__ __launch_bounds__(kBlock) void k_hist_sum(const double* partial, int n_wg, int nbins, double* out) {
  double v = 0.0;
  for (int w = threadIdx.x; w < n_wg; w += kBlock) v += partial[(u64)w * nbins + blockIdx.x];
  block_reduce_store<false>(v, out);
}

// ---- sparse view of the state: the v3 worker's rows (idx, re, im) with its pruning rule |re| > eps or |im| > eps
// (parallel_gate_applicator.py:372-374, state_manager.py:95-106), made on the device: a GHZ state of 30 qubits has two
// rows, not 16 GiB.  One pass counts, a second one appends the kept amplitudes (one atomic per wave reserves the slots;
// the rows arrive unordered and are sorted by index on the host).
__device__ __forceinline__ bool kept_amp(double2 v, double eps) { return fabs(v.x) > eps || fabs(v.y) > eps; }

__global__ __launch_bounds__(kBlock) void k_count_kept(const double2* p, u64 n, double eps, unsigned long long* count) {
  const u64 stride = (u64)gridDim.x * blockDim.x;
  unsigned long long mine = 0;
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) mine += kept_amp(p[i], eps) ? 1u : 0u;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off, 64);
  if ((threadIdx.x & 63) == 0 && mine) atomicAdd(count, mine);
}

__global__ __launch_bounds__(kBlock) void k_append_kept(const double2* p, u64 n, double eps, unsigned long long* cursor,
                                                        u64 capacity, u64* out_idx, double2* out_amp) {
  const u64 stride = (u64)gridDim.x * blockDim.x;
  const u64 rounds = (n + stride - 1) / stride;        // every lane runs every round (the ballot needs whole waves)
  for (u64 r = 0; r < rounds; ++r) {
    const u64 i = r * stride + (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const double2 v = i < n ? p[i] : make_double2(0.0, 0.0);
    const bool keep = i < n && kept_amp(v, eps);
    const unsigned long long mask = __ballot(keep);
    if (!mask) continue;
    const int lane = threadIdx.x & 63;
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(cursor, (unsigned long long)__popcll(mask));
    base = __shfl(base, 0, 64);
    if (keep) {
      const u64 at = base + (u64)__popcll(mask & ((1ull << lane) - 1));
      if (at < capacity) { out_idx[at] = i; out_amp[at] = v; }
    }
  }
}

// kind 0: GHZ, kind 1: GHZ+QFT closed form.  `base` = global index of amp 0.
struct BitPerm { unsigned char to_logical[64]; int active; };   // physical index bit -> logical qubit

__global__ __launch_bounds__(kBlock) void k_closed_form_err(const double2* p, u64 n, int kind,
                                                            int n_total, u64 base, double* partial,
                                                            const BitPerm perm) {
  const u64 stride = (u64)gridDim.x * blockDim.x;
  const double inv_n = exp2(-(double)n_total);
  const double amp = exp2(-0.5 * (double)(n_total + 1));
  const u64 last = (n_total >= 64) ? ~0ull : ((1ull << n_total) - 1);
  double worst = 0.0;
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    u64 y = base + i;
    if (perm.active) {                       // staged layout: logical index from the physical one
      const u64 x = y;
      y = 0;
      for (int b = 0; b < n_total; ++b) y |= ((x >> b) & 1ull) << perm.to_logical[b];
    }
    double er, ei;
    if (kind == 0) {
      er = (y == 0 || y == last) ? 0.70710678118654752440 : 0.0;
      ei = 0.0;
    } else {
      // exp(-2 pi i y / 2^n): y * 2^-n is exact in double for n <= 52
      double s, c;
      sincospi(-2.0 * ((double)y * inv_n), &s, &c);
      er = amp * (1.0 + c);
      ei = amp * s;
    }
    const double2 v = p[i];
    worst = max_keep_nan(worst, hypot(v.x - er, v.y - ei));
  }
  block_reduce_store<true>(worst, partial);
}

// ---- layout-aware fingerprint of a (partitioned, staged) state: sum_i amp_i * w(y_i) over the chunk's amplitudes whose
// LOGICAL index y_i passes the filter (y & sel_mask) == sel_value, with counter-based pseudo-random complex weights of y
// (two rounds of fp_mix, state_kernels.h, over y ^ mix(seed); real and imaginary part uniform in [-1, 1), exactly representable).
// A state that is right up to rounding gives the same value wherever its amplitudes live: a shard of a multi-GPU run in
// its staged layout, or the same index set of a one-GPU run (ref_dense.simulate semantics, ref_dense.py:44-57; layout
// permute_state, staging.py:639-658).  Slabs that trade places, a wrong permutation or a lost phase change it at O(1).
__global__ __launch_bounds__(kBlock) void k_fingerprint(const double2* p, u64 n, int n_total, u64 base, u64 seed_mix,
                                                        u64 sel_mask, u64 sel_value, double* partial, const BitPerm perm) {
  const u64 stride = (u64)gridDim.x * blockDim.x;
  double sr = 0.0, si = 0.0;
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    u64 y = base + i;
    if (perm.active) {
      const u64 x = y;
      y = 0;
      for (int b = 0; b < n_total; ++b) y |= ((x >> b) & 1ull) << perm.to_logical[b];
    }
    if ((y & sel_mask) != sel_value) continue;
    const u64 a = fp_mix(y ^ seed_mix), b2 = fp_mix(a);
    const double wr = (double)(a >> 11) * 0x1p-52 - 1.0, wi = (double)(b2 >> 11) * 0x1p-52 - 1.0;
    const double2 v = p[i];
    sr += v.x * wr - v.y * wi;
    si += v.x * wi + v.y * wr;
  }
  __shared__ double part[2 * (kBlock / 64)];
  sr = wave_sum(sr);
  si = wave_sum(si);
  if ((threadIdx.x & 63) == 0) { part[2 * (threadIdx.x >> 6)] = sr; part[2 * (threadIdx.x >> 6) + 1] = si; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double r = 0.0, im = 0.0;
    for (int w = 0; w < kBlock / 64; ++w) { r += part[2 * w]; im += part[2 * w + 1]; }
    partial[2 * blockIdx.x] = r;
    partial[2 * blockIdx.x + 1] = im;
  }
}

// ---- the chunk's device buffers
constexpr int kScratchDoubles = 8192;      // >= kReduceBlocks reduction partials, and a 64 x 64 complex matrix (dense blocks)
static_assert(kScratchDoubles >= kReduceBlocks, "the scratch holds the reduction partials");
static int ensure_scratch(qsim_chunk* c) {
  if (!c->scratch) {
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMalloc((void**)&c->scratch, sizeof(double) * kScratchDoubles));
  }
  return QSIM_OK;
}

// The readout workspace: one buffer per chunk, grown on demand, laid out by whichever readout call runs (every call ends
// with the stream synchronised, so no two layouts are alive at once).  A chunk holds the largest need so far, not the sum.
static int ensure_work(qsim_chunk* c, u64 bytes) {
  if (c->work_bytes >= bytes) return QSIM_OK;
  HIP_TRY(hipSetDevice(c->device));
  if (c->work) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipFree(c->work));
    c->work = nullptr;
    c->work_bytes = 0;
  }
  HIP_TRY(hipMalloc(&c->work, bytes));
  c->work_bytes = bytes;
  return QSIM_OK;
}

// ---- the finish of a call
// rows x n partials (one row per workgroup) -> n sums in a device slot, the rows in row order
static int sum_rows(qsim_chunk* c, const double* partial, unsigned rows, int n, double* dev_out) {
  hipLaunchKernelGGL(k_hist_sum, dim3(n), dim3(kBlock), 0, c->stream, partial, (int)rows, n, dev_out);
  HIP_TRY(hipGetLastError());
  return QSIM_OK;
}

// n doubles of the device on the host when it returns
static int fetch_doubles(qsim_chunk* c, const double* dev, u64 n, double* host) {
  HIP_TRY(hipMemcpyAsync(host, dev, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return QSIM_OK;
}

// the scratch's `grid` block partials of `width` interleaved values -> out[width]: long double sums in block order, or maxima
static int reduce_partials(qsim_chunk* c, unsigned grid, int width, bool max, double* out) {
  std::vector<double> host((size_t)width * grid);
  const int rc = fetch_doubles(c, c->scratch, host.size(), host.data());
  if (rc) return rc;
  for (int w = 0; w < width; ++w) {
    long double total = 0;
    double worst = 0;
    for (unsigned b = 0; b < grid; ++b) {
      const double v = host[(size_t)width * b + w];
      if (max) worst = max_keep_nan(worst, v);
      else total += v;
    }
    out[w] = max ? worst : (double)total;
  }
  return QSIM_OK;
}

constexpr int kHistWgBits = 11;            // qsim_probabilities: at most 2^11 workgroups (8 per CU)
constexpr u64 kHistDoubles = (256ull << kHistWgBits) + 256;   // partial histograms + the summed one
