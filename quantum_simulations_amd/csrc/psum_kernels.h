// psum_kernels.h -- a Pauli sum applied as an operator, out of place: dst = sum_t c_t P_t src (qsim_apply_pauli_sum).
// Part of the single translation unit qsim_hip.hip (included there after rot_kernels.h; not a standalone header).
//
// A Pauli string is two masks of physical index bits as in expect_kernels.h and rot_kernels.h: x = the bits that carry X
// or Y, z = the bits that carry Z or Y, ny = popcount(x & z), s(i) = (-1)^popcount(i & z):
//   (P psi)_j = i^ny s(j ^ x) psi_{j ^ x}.
// The terms of a sum commute under the sum, so the passes are those of plan_expectation (expect_kernels.h): terms
// grouped by the tile their x fits.  The first pass WRITES dst (whatever dst held does not matter), every later pass
// ACCUMULATES into it; the template flag ACC selects the form.
//
// Tile pass (k_psum_tile): the tile walk, the off[] offsets and the base deposit of k_rot_tile.  The src tile goes into
// LDS and is only read from then on: a thread keeps the kLoads results of the slots j it loaded in registers and adds
// g s(j ^ xi) tile[j ^ xi] per term, g = c_t i^ny (outer sign) once per tile and term.  Because the tile is never
// written between the fill and the next refill, NO barrier separates two terms (k_rot_tile needs one: its rotations
// update the tile in place and do not commute); the two barriers per tile are the one after the fill and the one in
// front of the next refill.  The term table is read through the constant address space at wave-uniform addresses:
// scalar loads.  With ACC the old dst values are loaded before the term loop, so their latency hides under it.  The
// results go to dst + (base | off[it]), whole 128-byte lines as they were loaded.  Which term count turns the pass from
// HBM-bound to LDS-bound is measured in profiles/r18_hamiltonian_probe.json.
//
// Wide pass (k_psum_wide): one term whose x does not fit a tile with the line bits; each lane computes
// dst[j] (+)= g s(j ^ x) src[j ^ x].  Correctness, not speed.
struct PauliTerm {       // one term of a tile pass in tile coordinates (inner bit b <-> physical bit tile_bit[b])
  u64 zo;                // z outside the tile (physical bits): the outer sign
  double gr, gi;         // g = c_t i^ny (qsim_overlap_pauli: i^ny)
  unsigned xi, zi;       // x and z & T compressed onto the tile bits
};

struct PsumArgs {
  double2* dst;
  const double2* src;
  const PauliTerm* terms;
  u64 n_tiles;           // 2^(k - tb)
  u64 outer_mask;        // physical bits outside the tile (outer index bit j <-> the j-th set bit)
  int tile_bit[kExpTileBits];
  int tb;                // tile bits
  int n_terms;           // <= kExpMaxTerms
};

template <bool NT, bool ACC>
__global__ __launch_bounds__(kBlock) void k_psum_tile(const PsumArgs a) {
  constexpr int kTile = 1 << kExpTileBits;
  constexpr int kLoads = kTile / kBlock;
  __shared__ double2 tile[kTile];
  const int S = 1 << a.tb;
  const int tid = threadIdx.x;
  typedef __attribute__((address_space(4))) const PauliTerm cterm_t;    // scalar loads, as in k_rot_tile
  cterm_t* const terms = (cterm_t*)(unsigned long long)a.terms;
  u64 off[kLoads];                                  // physical offsets of the amplitudes this thread owns (every tile)
#pragma unroll
  for (int it = 0; it < kLoads; ++it) {
    const int j = tid + it * kBlock;
    u64 o = 0;
    for (int b = 0; b < a.tb; ++b) o |= (u64)((j >> b) & 1) << a.tile_bit[b];
    off[it] = o;
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
      if (tid + it * kBlock < S) x[it] = ld_amp<NT>(a.src + (base | off[it]));
    __syncthreads();                                // (every thread is past the last term of the previous tile)
#pragma unroll
    for (int it = 0; it < kLoads; ++it)
      if (tid + it * kBlock < S) tile[tid + it * kBlock] = x[it];
    __syncthreads();                                // the tile is filled; it is only read until the next refill
    double2 acc[kLoads];
#pragma unroll
    for (int it = 0; it < kLoads; ++it) {
      acc[it] = make_double2(0.0, 0.0);
      if (ACC && tid + it * kBlock < S) acc[it] = ld_amp<NT>(a.dst + (base | off[it]));
    }
    for (int t = 0; t < a.n_terms; ++t) {
      const u64 zo = terms[t].zo;                   // wave-uniform addresses: scalar loads
      const unsigned xi = terms[t].xi, zi = terms[t].zi;
      const bool neg = __popcll(base & zo) & 1;     // the sign over the outer bits: one per tile and term
      const double gr = neg ? -terms[t].gr : terms[t].gr, gi = neg ? -terms[t].gi : terms[t].gi;
#pragma unroll
      for (int it = 0; it < kLoads; ++it) {
        const unsigned p = ((unsigned)(tid + it * kBlock) ^ xi) & (unsigned)(S - 1);
        const double2 w = tile[p];
        const bool sp = __popc(p & zi) & 1;
        const double qr = sp ? -gr : gr, qi = sp ? -gi : gi;
        acc[it].x = fma(qr, w.x, fma(-qi, w.y, acc[it].x));
        acc[it].y = fma(qr, w.y, fma(qi, w.x, acc[it].y));
      }
    }
#pragma unroll
    for (int it = 0; it < kLoads; ++it)
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

// i^ny of a string: 1, i, -1, -i for ny = 0..3
static void pauli_phase(u64 x, u64 z, double* gr, double* gi) {
  static const double kr[4] = {1.0, 0.0, -1.0, 0.0}, ki[4] = {0.0, 1.0, 0.0, -1.0};
  const int ny = __builtin_popcountll(x & z) & 3;
  *gr = kr[ny];
  *gi = ki[ny];
}

// What qsim_apply_pauli_sum and qsim_overlap_pauli share on the host: the plan, the result slot of every term (terms in
// pass order), the table in tile coordinates with g = coeff * i^ny (coeffs null: i^ny), and the term of every wide pass.
struct PauliPasses {
  ExpPlan plan;
  std::vector<int> first;          // first table entry of every pass (+ the end)
  std::vector<int> slot;           // table entry of term t
  std::vector<int> wide_term;      // per pass: the term of a wide pass, else -1
  std::vector<PauliTerm> table;
};

static int pauli_passes(int k, int n_terms, const uint64_t* x_masks, const uint64_t* z_masks, const double* coeffs, PauliPasses* pp) {
  const int rc = plan_expectation(k, n_terms, x_masks, &pp->plan);
  if (rc) return rc;
  const ExpPlan& p = pp->plan;
  const int np = (int)p.tile.size();
  pp->first.assign((size_t)np + 1, 0);
  for (int q = 0; q < np; ++q) pp->first[(size_t)q + 1] = pp->first[(size_t)q] + p.count[(size_t)q];
  std::vector<int> fill(pp->first.begin(), pp->first.end() - 1);
  pp->slot.assign((size_t)n_terms, 0);
  for (int t = 0; t < n_terms; ++t) pp->slot[(size_t)t] = fill[(size_t)p.pass_of[(size_t)t]]++;
  pp->table.assign((size_t)n_terms, PauliTerm());
  if (n_terms) std::memset(pp->table.data(), 0, sizeof(PauliTerm) * pp->table.size());
  pp->wide_term.assign((size_t)np, -1);
  for (int t = 0; t < n_terms; ++t) {
    const u64 T = p.tile[(size_t)p.pass_of[(size_t)t]];
    const u64 x = x_masks[t], z = z_masks[t];
    PauliTerm& e = pp->table[(size_t)pp->slot[(size_t)t]];
    pauli_phase(x, z, &e.gr, &e.gi);
    if (coeffs) { e.gr *= coeffs[t]; e.gi *= coeffs[t]; }
    if (!T && x) {                                  // wide: the masks go as launch arguments
      pp->wide_term[(size_t)p.pass_of[(size_t)t]] = t;
      continue;
    }
    e.xi = (unsigned)exp_pext(x, T);
    e.zi = (unsigned)exp_pext(z & T, T);
    e.zo = z & ~T;
  }
  return QSIM_OK;
}

// the tile walk of a pass with tile bits T on a chunk of k index bits, as launch arguments
template <class Args>
static void pauli_tile_walk(int k, u64 T, Args* a) {
  a->tb = __builtin_popcountll(T);
  for (int b = 0, j = 0; b < k; ++b)
    if ((T >> b) & 1) a->tile_bit[j++] = b;
  a->outer_mask = ((1ull << k) - 1) & ~T;
  a->n_tiles = 1ull << (k - a->tb);
}
