// state_kernels.h -- kernels that write or copy a whole state: fill, random fill, scale, copy, complex64 conversion.
// Part of the single translation unit qsim_hip.hip (included there, in order; not a standalone header).
__global__ void k_fill_zero(double2* p, u64 n, int set0) {
  const u64 stride = (u64)gridDim.x * blockDim.x;
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    p[i] = make_double2((i == 0 && set0) ? 1.0 : 0.0, 0.0);
}

// The one mixing function (splitmix64's finaliser over a counter): the random fill, the fingerprint's weights and the
// fingerprint's seed on the host.
__host__ __device__ __forceinline__ u64 fp_mix(u64 x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// amplitude i = (u(2i), u(2i+1)), u(j) = (fp_mix(seed + j) >> 11) * 2^-52 - 1 in [-1, 1)
__global__ void k_fill_random(double2* p, u64 n, u64 seed) {
  const u64 stride = (u64)gridDim.x * blockDim.x;
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const double re = (double)(fp_mix(seed + 2 * i) >> 11) * (1.0 / 4503599627370496.0) - 1.0;
    const double im = (double)(fp_mix(seed + 2 * i + 1) >> 11) * (1.0 / 4503599627370496.0) - 1.0;
    p[i] = make_double2(re, im);
  }
}

__global__ void k_scale(double2* p, u64 n, double s) {
  const u64 stride = (u64)gridDim.x * blockDim.x;
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    double2 v = p[i];
    p[i] = make_double2(v.x * s, v.y * s);
  }
}

// NT: streaming (non-temporal) accesses for copies larger than the Infinity Cache -- the same cache
// policy the gate kernels use; this copy is also bench.py's same-run device-to-device ceiling.
// One-shot grid, ITEMS 16-byte elements per thread, XCD-contiguous block order (the shape of the gate
// kernels: grid-stride loops are 5-8 % slower, tools/bw_probe.hip).
template <bool NT, int ITEMS>
__global__ __launch_bounds__(kBlock) void k_copy(double2* __restrict__ dst, const double2* __restrict__ src, u64 n) {
  const u64 first = (logical_block<true>() * ITEMS) * kBlock + threadIdx.x;
  double2 v[ITEMS];
#pragma unroll
  for (int r = 0; r < ITEMS; ++r) if (first + (u64)r * kBlock < n) v[r] = ld_amp<NT>(src + first + (u64)r * kBlock);
#pragma unroll
  for (int r = 0; r < ITEMS; ++r) if (first + (u64)r * kBlock < n) st_amp<NT>(dst + first + (u64)r * kBlock, v[r]);
}

// ---- complex64 <-> complex128 on the device: the reference's chunk files are complex64 (storage/block_store.py:11),
// so an export rounds on the GPU and moves 8 B per amplitude over PCIe instead of 16 (round to nearest even, what
// numpy's astype(complex64) does)
__global__ __launch_bounds__(kBlock) void k_to_c64(float2* __restrict__ dst, const double2* __restrict__ src, u64 n) {
  const u64 stride = (u64)gridDim.x * blockDim.x;
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const double2 v = src[i];
    dst[i] = make_float2(__double2float_rn(v.x), __double2float_rn(v.y));
  }
}
__global__ __launch_bounds__(kBlock) void k_from_c64(double2* __restrict__ dst, const float2* __restrict__ src, u64 n) {
  const u64 stride = (u64)gridDim.x * blockDim.x;
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float2 v = src[i];
    dst[i] = make_double2((double)v.x, (double)v.y);
  }
}

static unsigned stream_grid(u64 n) {
  const u64 want = (n + kBlock - 1) / kBlock;
  return (unsigned)std::min<u64>(std::max<u64>(want, 1), 8192);
}
