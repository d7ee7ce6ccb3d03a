// pauli_tile.h -- what the four Pauli-string families share: expectation values (expect_kernels.h), rotations
// (rot_kernels.h), a sum applied out of place (psum_kernels.h) and two-state overlaps (ovl_kernels.h).
// Part of the single translation unit qsim_hip.hip (included there after dense_kernels.h; not a standalone header).
//
// A Pauli string is two masks of physical index bits: x = the bits that carry X or Y, z = the bits that carry Z or Y.
// With ny = popcount(x & z) (Y = i X Z) and s(i) = (-1)^popcount(i & z):   (P psi)_j = i^ny s(j ^ x) psi_{j ^ x}.
//
// The tile walk: a pass has a set T of tile bits (<= kExpTileBits, the line bits 0..2 among them: every global access is
// a whole 128-byte line).  A tile is the 2^|T| amplitudes with fixed outer bits; a workgroup walks tiles with a
// grid-stride loop over the outer index o.  Thread tid owns the slots j = tid + it * kBlock of every tile: tile_offsets
// spreads j over the tile bits once, tile_base deposits o on the outer bits once per tile, tile_load brings the slots
// into registers and tile_fill puts them into LDS.  The barriers around tile_fill stay in the kernels: they differ.
// Every term of the pass has its x inside T, so with a tile in LDS it is evaluated from LDS alone.  z need not lie in T:
// s(i) = s(inner, z & T) s(outer, z & ~T), and x moves no outer bit, so the outer sign is one factor per tile and term.
// A term whose x does not fit a tile with the line bits gets a wide pass of its own (correctness, not speed).
constexpr int kExpTileBits = 11;                    // the fused pass's tile width: 2^11 amplitudes = 32 KiB of LDS
constexpr int kExpMaxTerms = 1024;                  // terms per tile launch (the planner opens a new pass beyond)
constexpr int kExpSlots = kExpMaxTerms / kBlock;    // terms one thread evaluates at most
constexpr int kExpMaxWg = 1024;                     // workgroups per launch: 4 per CU at 32 KiB of LDS each
constexpr int kExpLineBits = 3;                     // 128-byte lines: 8 amplitudes
constexpr int kExpTile = 1 << kExpTileBits;
constexpr int kExpLoads = kExpTile / kBlock;        // slots of a tile per thread

struct TileWalk {        // part of the launch arguments of every tile kernel
  u64 n_tiles;           // 2^(k - tb)
  u64 outer_mask;        // physical bits outside the tile (outer index bit j <-> the j-th set bit)
  int tile_bit[kExpTileBits];   // inner bit b <-> physical bit tile_bit[b]
  int tb;                // tile bits
};

struct PauliTerm {       // one term of a tile pass in tile coordinates; 48 bytes
  u64 zo;                // z outside the tile (physical bits): the outer sign
  double f0, f1;         // the family's factors (PauliRule; each kernel header says what it keeps here)
  unsigned xi, zi;       // x and z & T compressed onto the tile bits
  double f2;
  int h;                 // the top bit of xi (pairs run over the half with it clear); -1: x = 0
  int pad_;
};
// A family's table on the device holds the leading bytes of every record that its kernel reads, at that stride: sum and
// overlap the first 32 (one s_load_dwordx8 per term in k_psum_tile), expectation and rotations the whole record.  With
// 48-byte entries k_psum_tile passes of 512 terms (24 KiB a walk instead of 16) and k_ovl_tile passes of 32 and more
// terms measured 2-3 % slower (profiles/r20_pauli_refactor_ab.txt).
constexpr int kSumStride = 32, kTermStride = sizeof(PauliTerm);

// entry t of a table of STRIDE-byte entries, as far as the stride holds it
template <int STRIDE>
__device__ __forceinline__ void term_load(const PauliTerm* table, int t, PauliTerm* e) {
  const PauliTerm* p = reinterpret_cast<const PauliTerm*>(reinterpret_cast<const char*>(table) + (size_t)t * STRIDE);
  e->zo = p->zo;
  e->f0 = p->f0;
  e->f1 = p->f1;
  e->xi = p->xi;
  e->zi = p->zi;
  if (STRIDE > 32) e->h = p->h;
}

__device__ __forceinline__ void tile_offsets(const TileWalk& w, u64* off) {   // physical offsets of this thread's slots
#pragma unroll
  for (int it = 0; it < kExpLoads; ++it) {
    const int j = (int)threadIdx.x + it * kBlock;
    u64 o = 0;
    for (int b = 0; b < w.tb; ++b) o |= (u64)((j >> b) & 1) << w.tile_bit[b];
    off[it] = o;
  }
}

__device__ __forceinline__ u64 tile_base(u64 outer_mask, u64 o) {   // the outer index o deposited on the outer bits
  u64 base = 0, m = outer_mask;
  while (m) {
    const u64 low = m & (~m + 1);
    if (o & 1) base |= low;
    o >>= 1;
    m ^= low;
  }
  return base;
}

template <bool NT>
__device__ __forceinline__ void tile_load(const double2* amp, u64 base, const u64* off, int S, double2* x) {
#pragma unroll
  for (int it = 0; it < kExpLoads; ++it)
    if ((int)threadIdx.x + it * kBlock < S) x[it] = ld_amp<NT>(amp + (base | off[it]));
}

__device__ __forceinline__ void tile_fill(double2* tile, int S, const double2* x) {
#pragma unroll
  for (int it = 0; it < kExpLoads; ++it)
    if ((int)threadIdx.x + it * kBlock < S) tile[(int)threadIdx.x + it * kBlock] = x[it];
}

// ---- host: the pass plan (pure, no GPU)
// A term whose x and the line bits exceed K = min(k, kExpTileBits) bits gets a wide pass of its own (tile mask 0); any
// other joins a tile pass that holds fewer than kExpMaxTerms terms and whose tile bits (the union of its terms' x and
// the line bits) stay within K with x added, else it opens one.  Which pass is tried is the family's rule:
//   commuting terms (expectation, sum, overlap): first fit, deterministic.  Terms with x != 0 in input order go into
//     the first pass that takes them; terms with x = 0 then fill the tile passes in order.  Passes: the tile passes in
//     creation order, then the wide passes in term order.
//   ordered (rotations do not commute): the list is walked once and only the last pass is tried; a wide pass closes
//     it.  pass_of is non-decreasing.
// Finished tiles are completed to K bits with the lowest free bits.
struct PauliPlan {
  std::vector<int32_t> pass_of;   // per term
  std::vector<u64> tile;          // per pass (0: wide)
  std::vector<int> count;         // terms per pass
};

static int plan_pauli(bool ordered, int k, int n, const uint64_t* x, PauliPlan* p) {
  const char* const what = ordered ? "qsim_plan_pauli_rotations" : "qsim_plan_expectation";
  if (k < 0 || k > 63) return fail(QSIM_ERR_INVALID, "%s: %d local qubits", what, k);
  if (n < 0) return fail(QSIM_ERR_INVALID, "%s: %s = %d", what, ordered ? "n" : "n_terms", n);
  if (n > 0 && !x) return fail(QSIM_ERR_INVALID, "%s: null x_masks", what);
  const u64 all = (1ull << k) - 1;
  for (int t = 0; t < n; ++t)
    if (x[t] & ~all)
      return fail(QSIM_ERR_NONLOCAL, "%s %d: X/Y on index bit %d >= log2(chunk_size)=%d", ordered ? "rotation" : "term", t,
                  63 - __builtin_clzll(x[t] & ~all), k);
  const int K = std::min(k, kExpTileBits);
  const u64 line = (1ull << std::min(k, kExpLineBits)) - 1;
  p->pass_of.assign((size_t)n, -1);
  p->tile.clear();
  p->count.clear();
  const auto wide = [&](int t) { return __builtin_popcountll(x[t] | line) > K; };
  const auto takes = [&](size_t q, int t) { return p->count[q] < kExpMaxTerms && __builtin_popcountll(p->tile[q] | x[t]) <= K; };
  const auto put = [&](int t, size_t q, u64 T) {    // term t into pass q: a new one with tile bits T when q is the end
    if (q == p->tile.size()) { p->tile.push_back(T); p->count.push_back(0); }
    ++p->count[q];
    p->pass_of[(size_t)t] = (int32_t)q;
  };
  if (ordered) {
    bool open = false;                              // the last pass is a tile pass that may still take rotations
    for (int t = 0; t < n; ++t) {
      const size_t end = p->tile.size();
      if (wide(t)) { put(t, end, 0); open = false; continue; }
      const size_t q = open && takes(end - 1, t) ? end - 1 : end;
      put(t, q, line);
      p->tile[q] |= x[t];
      open = true;
    }
  } else {
    std::vector<int> wides;
    for (int fill = 0; fill < 2; ++fill)
      for (int t = 0; t < n; ++t) {
        if ((x[t] == 0) != (fill == 1)) continue;
        if (wide(t)) { wides.push_back(t); continue; }
        size_t q = 0;
        while (q < p->tile.size() && !takes(q, t)) ++q;
        put(t, q, line);
        p->tile[q] |= x[t];
      }
    for (int t : wides) put(t, p->tile.size(), 0);
  }
  for (u64& m : p->tile)
    if (m)
      for (int b = 0; b < k && __builtin_popcountll(m) < K; ++b) m |= 1ull << b;
  return QSIM_OK;
}

// The factors of a term, in double on the host, all from Re i^m = 1, 0, -1, 0 (Im i^m = Re i^(m + 3)):
//   kPauliExpect:    f = (cr, ci), value = cr sum s Re(c) + ci sum s Im(c): Re(i^ny c), twice that for x != 0 (the pairs)
//   kPauliRotation:  f = (cos(v), fr, fi), fr + i fi = -i sin(v) i^ny = sin(v) i^(ny + 3); v = theta
//   kPauliSum:       f = (gr, gi), gr + i gi = v i^ny; v = the coefficient, or null: 1
enum PauliRule { kPauliExpect, kPauliRotation, kPauliSum };

static void pauli_factors(PauliRule rule, u64 x, u64 z, const double* v, PauliTerm* e) {
  static const double re[4] = {1.0, 0.0, -1.0, 0.0};
  const int ny = __builtin_popcountll(x & z);
  if (rule == kPauliExpect) {
    const double two = x ? 2.0 : 1.0;
    e->f0 = two * re[ny & 3];
    e->f1 = two * re[(ny + 1) & 3];                // -Im i^ny = Re i^(ny + 1)
  } else if (rule == kPauliRotation) {
    const double s = std::sin(*v);
    e->f0 = std::cos(*v);
    e->f1 = re[(ny + 3) & 3] * s;
    e->f2 = re[(ny + 2) & 3] * s;
  } else {
    e->f0 = re[ny & 3];
    e->f1 = re[(ny + 3) & 3];
    if (v) { e->f0 *= *v; e->f1 *= *v; }
  }
}

static u64 exp_pext(u64 v, u64 mask) {
  u64 r = 0;
  for (int j = 0; mask; mask &= mask - 1, ++j)
    if (v & mask & (~mask + 1)) r |= 1ull << j;
  return r;
}

// ---- host: from the plan to the term table and the launch arguments
// What the four calls share: the plan, the table entry of every term (terms in pass order; for rotations that is list
// order), the table in tile coordinates with the family's factors (v: thetas or coefficients, or null) as the device
// reads it (entries of `stride` bytes), and the term of every wide pass (its masks go as launch arguments, its factors
// are those of its table entry).
struct PauliPasses {
  PauliPlan plan;
  std::vector<int> first;          // first table entry of every pass (+ the end)
  std::vector<int> slot;           // table entry of term t
  std::vector<int> wide_term;      // per pass: the term of a wide pass, else -1
  int stride;                      // kSumStride or kTermStride
  std::vector<char> table;         // n entries of `stride` bytes: the leading bytes of a PauliTerm
  PauliTerm entry(int i) const {
    PauliTerm e;
    std::memset(&e, 0, sizeof e);
    std::memcpy(&e, table.data() + (size_t)i * stride, (size_t)stride);
    return e;
  }
  const PauliTerm* at(const void* dev_table, int i) const {   // entry i of the table's copy on the device
    return reinterpret_cast<const PauliTerm*>(static_cast<const char*>(dev_table) + (size_t)i * stride);
  }
};

static int pauli_passes(PauliRule rule, int k, int n, const uint64_t* x_masks, const uint64_t* z_masks, const double* v, PauliPasses* pp) {
  const int rc = plan_pauli(rule == kPauliRotation, k, n, x_masks, &pp->plan);
  if (rc) return rc;
  const PauliPlan& p = pp->plan;
  const int np = (int)p.tile.size();
  pp->first.assign((size_t)np + 1, 0);
  for (int q = 0; q < np; ++q) pp->first[(size_t)q + 1] = pp->first[(size_t)q] + p.count[(size_t)q];
  std::vector<int> fill(pp->first.begin(), pp->first.end() - 1);
  pp->slot.assign((size_t)n, 0);
  pp->stride = rule == kPauliSum ? kSumStride : kTermStride;
  pp->table.assign((size_t)n * pp->stride, 0);
  pp->wide_term.assign((size_t)np, -1);
  for (int t = 0; t < n; ++t) {
    const int q = p.pass_of[(size_t)t];
    const u64 T = p.tile[(size_t)q], x = x_masks[t], z = z_masks[t];
    PauliTerm e;
    std::memset(&e, 0, sizeof e);
    pauli_factors(rule, x, z, v ? v + t : nullptr, &e);
    if (!T && x) {                                  // wide
      pp->wide_term[(size_t)q] = t;
    } else {
      e.xi = (unsigned)exp_pext(x, T);
      e.zi = (unsigned)exp_pext(z & T, T);
      e.zo = z & ~T;
      e.h = e.xi ? 31 - __builtin_clz(e.xi) : -1;
    }
    pp->slot[(size_t)t] = fill[(size_t)q]++;
    std::memcpy(pp->table.data() + (size_t)pp->slot[(size_t)t] * pp->stride, &e, (size_t)pp->stride);
  }
  return QSIM_OK;
}

// the tile walk of a pass with tile bits T on a chunk of k index bits
static TileWalk tile_walk(int k, u64 T) {
  TileWalk w;
  std::memset(&w, 0, sizeof w);
  w.tb = __builtin_popcountll(T);
  for (int b = 0, j = 0; b < k; ++b)
    if ((T >> b) & 1) w.tile_bit[j++] = b;
  w.outer_mask = ((1ull << k) - 1) & ~T;
  w.n_tiles = 1ull << (k - w.tb);
  return w;
}

// threads per term of k_expect_tile and k_ovl_tile: a power of two, slices * min(n_terms, 256) <= 256
static int pauli_slices(int n_terms) {
  int slices = 1;
  while (slices * 2 * n_terms <= kBlock) slices *= 2;
  return slices;
}

// workgroups of a wide pass over `items` work items
static unsigned pauli_wide_grid(u64 items) { return (unsigned)std::min<u64>(std::max<u64>(items / kBlock, 1), kExpMaxWg); }
