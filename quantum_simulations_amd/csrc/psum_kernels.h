// psum_kernels.h -- a Pauli sum applied as an operator, out of place: dst = sum_t c_t P_t src (qsim_apply_pauli_sum).
// Part of the single translation unit qsim_hip.hip (included there after rot_kernels.h; not a standalone header).
//
// Masks, ny and s(i) as in pauli_tile.h:   (P psi)_j = i^ny s(j ^ x) psi_{j ^ x}.
// The terms of a sum commute under the sum, so the passes are those of qsim_plan_expectation: terms grouped by the tile
// their x fits.  The first pass WRITES dst (whatever dst held does not matter), every later pass
// ACCUMULATES into it; the template flag ACC selects the form.
//
// Tile pass (k_psum_tile): the tile walk of pauli_tile.h, from src to dst.  A term keeps (gr, gi) in f0, f1
// (kPauliSum: g = c_t i^ny).  The src tile goes into LDS and is only read from then on: a thread keeps the kExpLoads
// results of the slots j it loaded in registers and adds g s(j ^ xi) tile[j ^ xi] per term, the outer sign on g once per
// tile and term.  Because the tile is never
// written between the fill and the next refill, NO barrier separates two terms (k_rot_tile needs one: its rotations
// update the tile in place and do not commute); the two barriers per tile are the one after the fill and the one in
// front of the next refill.  The term table is read through the constant address space at wave-uniform addresses:
// scalar loads.  With ACC the old dst values are loaded before the term loop, so their latency hides under it.  The
// results go to dst + (base | off[it]), whole 128-byte lines as they were loaded.  Which term count turns the pass from
// HBM-bound to LDS-bound is measured in profiles/r18_hamiltonian_probe.json.
//
// Wide pass (k_psum_wide): one term whose x does not fit a tile with the line bits; each lane computes
// dst[j] (+)= g s(j ^ x) src[j ^ x].  Correctness, not speed.
struct PsumArgs {
  double2* dst;
  const double2* src;
  const PauliTerm* terms;   // entries of kSumStride bytes
  TileWalk w;
  int n_terms;           // <= kExpMaxTerms
};

template <bool NT, bool ACC>
__global__ __launch_bounds__(kBlock) void k_psum_tile(const PsumArgs a) {
  __shared__ double2 tile[kExpTile];
  const int S = 1 << a.w.tb;
  const int tid = threadIdx.x;
  typedef __attribute__((address_space(4))) const PauliTerm cterm_t;    // scalar loads, as in k_rot_tile
  const unsigned long long terms = (unsigned long long)a.terms;
  u64 off[kExpLoads];
  tile_offsets(a.w, off);
  for (u64 o = blockIdx.x; o < a.w.n_tiles; o += gridDim.x) {
    const u64 base = tile_base(a.w.outer_mask, o);
    double2 x[kExpLoads];
    tile_load<NT>(a.src, base, off, S, x);
    __syncthreads();                                // (every thread is past the last term of the previous tile)
    tile_fill(tile, S, x);
    __syncthreads();                                // the tile is filled; it is only read until the next refill
    double2 acc[kExpLoads];
#pragma unroll
    for (int it = 0; it < kExpLoads; ++it) {
      acc[it] = make_double2(0.0, 0.0);
      if (ACC && tid + it * kBlock < S) acc[it] = ld_amp<NT>(a.dst + (base | off[it]));
    }
    for (int t = 0; t < a.n_terms; ++t) {
      cterm_t& e = *(cterm_t*)(terms + (unsigned long long)t * kSumStride);   // wave-uniform addresses: scalar loads
      const u64 zo = e.zo;
      const unsigned xi = e.xi, zi = e.zi;
      const bool neg = __popcll(base & zo) & 1;     // the sign over the outer bits: one per tile and term
      const double gr = neg ? -e.f0 : e.f0, gi = neg ? -e.f1 : e.f1;
#pragma unroll
      for (int it = 0; it < kExpLoads; ++it) {
        const unsigned p = ((unsigned)(tid + it * kBlock) ^ xi) & (unsigned)(S - 1);
        const double2 w = tile[p];
        const bool sp = __popc(p & zi) & 1;
        const double qr = sp ? -gr : gr, qi = sp ? -gi : gi;
        acc[it].x = fma(qr, w.x, fma(-qi, w.y, acc[it].x));
        acc[it].y = fma(qr, w.y, fma(qi, w.x, acc[it].y));
      }
    }
#pragma unroll
    for (int it = 0; it < kExpLoads; ++it)
      if (tid + it * kBlock < S) st_amp<NT>(a.dst + (base | off[it]), acc[it]);
  }
}

struct PsumWideArgs {
  double2* dst;
  const double2* src;
  u64 n;                 // amplitudes
  u64 x, z;
  double gr, gi;         // c_t i^ny
};

template <bool NT, bool ACC>
__global__ __launch_bounds__(kBlock) void k_psum_wide(const PsumWideArgs a) {
  const u64 stride = (u64)gridDim.x * kBlock;
  for (u64 j = (u64)blockIdx.x * kBlock + threadIdx.x; j < a.n; j += stride) {
    const u64 p = j ^ a.x;
    const double2 w = ld_amp<NT>(a.src + p);
    const bool sp = __popcll(p & a.z) & 1;
    const double qr = sp ? -a.gr : a.gr, qi = sp ? -a.gi : a.gi;
    double2 v = make_double2(0.0, 0.0);
    if (ACC) v = ld_amp<NT>(a.dst + j);
    v.x = fma(qr, w.x, fma(-qi, w.y, v.x));
    v.y = fma(qr, w.y, fma(qi, w.x, v.y));
    st_amp<NT>(a.dst + j, v);
  }
}
