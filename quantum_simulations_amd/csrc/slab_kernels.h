// slab_kernels.h -- the pack / unpack / swap kernels of the re-layout (abi_relayout.h).
// Part of the single translation unit qsim_hip.hip (included by abi_relayout.h; not a standalone header).
// dst[j] = src[insert(j, bit, value)]  /  inverse
__global__ void k_pack_half(double2* __restrict__ dst, const double2* __restrict__ src, u64 n_half,
                            int bit, u64 value_off) {
  const u64 stride = (u64)gridDim.x * blockDim.x;
  for (u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x; j < n_half; j += stride) {
    const u64 i = (((j >> bit) << (bit + 1)) | (j & ((1ull << bit) - 1))) | value_off;
    dst[j] = src[i];
  }
}
__global__ void k_unpack_half(double2* __restrict__ dst, const double2* __restrict__ src, u64 n_half,
                              int bit, u64 value_off) {
  const u64 stride = (u64)gridDim.x * blockDim.x;
  for (u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x; j < n_half; j += stride) {
    const u64 i = (((j >> bit) << (bit + 1)) | (j & ((1ull << bit) - 1))) | value_off;
    dst[i] = src[j];
  }
}

// slab gather / scatter for the all-to-all re-layout: j runs over the 2^(k-m) amplitudes whose
// bits `pos` equal the pattern folded into value_off
__global__ void k_pack_bits(double2* __restrict__ dst, const double2* __restrict__ src, u64 n_slab,
                            int npos, int p0, int p1, int p2, u64 value_off) {
  const u64 stride = (u64)gridDim.x * blockDim.x;
  for (u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x; j < n_slab; j += stride)
    dst[j] = ld_amp<true>(src + (expand_index(j, npos, p0, p1, p2) | value_off));
}
__global__ void k_unpack_bits(double2* __restrict__ dst, const double2* __restrict__ src, u64 n_slab,
                              int npos, int p0, int p1, int p2, u64 value_off) {
  const u64 stride = (u64)gridDim.x * blockDim.x;
  for (u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x; j < n_slab; j += stride)
    dst[expand_index(j, npos, p0, p1, p2) | value_off] = ld_amp<true>(src + j);
}

// All slabs in one pass: amplitude i goes to slab pattern(i) at its compressed index (and back).
// Consecutive lanes read consecutive amplitudes, and the <= 8 slabs a wave feeds each receive a
// contiguous run, so reads and writes are whole 128-B lines for ANY choice of bits -- the
// per-pattern kernels above touch 16 B of every line when a selected bit is below 3
// (tools/relayout_probe.py: 0.7-1.0 TB/s instead of 4.5-5; the gather side of unpack with lanes of
// one line 8 apart still runs at 2.6-3.5 TB/s).  `skip` = the pattern that stays.
__device__ __forceinline__ u64 drop_bit(u64 x, int p) { return ((x >> (p + 1)) << p) | (x & ((1ull << p) - 1)); }
template <bool PACK>
__global__ void k_slabs_all(double2* __restrict__ state, double2* __restrict__ buf, u64 n, int m,
                            int b0, int b1, int b2, int s_hi, int s_mid, int s_lo, int slab_bits, int skip,
                            int n_piece_bits, int pb0, int pb1, int pb2, int piece) {
  // A piece = the amplitudes whose top `n_piece_bits` non-selected index bits equal `piece`: the
  // same contiguous sub-range of every slab, so the exchange can be pipelined piece by piece.
  const u64 stride = (u64)gridDim.x * blockDim.x;
  for (u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += stride) {
    u64 i = t;
    if (n_piece_bits > 0) i = (((i >> pb0) << (pb0 + 1)) | (i & ((1ull << pb0) - 1))) | ((u64)(piece & 1) << pb0);
    if (n_piece_bits > 1) i = (((i >> pb1) << (pb1 + 1)) | (i & ((1ull << pb1) - 1))) | ((u64)((piece >> 1) & 1) << pb1);
    if (n_piece_bits > 2) i = (((i >> pb2) << (pb2 + 1)) | (i & ((1ull << pb2) - 1))) | ((u64)((piece >> 2) & 1) << pb2);
    int p = (int)((i >> b0) & 1);
    if (m > 1) p |= (int)((i >> b1) & 1) << 1;
    if (m > 2) p |= (int)((i >> b2) & 1) << 2;
    if (p == skip) continue;
    u64 j = i;
    if (m > 2) j = drop_bit(j, s_hi);
    if (m > 1) j = drop_bit(j, s_mid);
    j = drop_bit(j, s_lo);
    double2* const slot = buf + (((u64)p << slab_bits) | j);
    if (PACK) st_amp<true>(slot, ld_amp<true>(state + i));
    else st_amp<true>(state + i, ld_amp<true>(slot));
  }
}

// exchange slab (bits pos == a_off pattern) of chunk A with slab (bits pos == b_off pattern) of chunk B
__global__ void k_swap_slabs(double2* __restrict__ a, double2* __restrict__ b, u64 n_slab,
                             int npos, int p0, int p1, int p2, u64 a_off, u64 b_off) {
  const u64 stride = (u64)gridDim.x * blockDim.x;
  for (u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x; j < n_slab; j += stride) {
    const u64 e = expand_index(j, npos, p0, p1, p2);
    const double2 x = a[e | a_off], y = b[e | b_off];
    a[e | a_off] = y;
    b[e | b_off] = x;
  }
}
