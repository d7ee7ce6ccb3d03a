// rot_kernels.h -- Pauli rotations exp(-i theta P) (qsim_plan_pauli_rotations, qsim_apply_pauli_rotations).
// Part of the single translation unit qsim_hip.hip (included there after expect_kernels.h; not a standalone header).
//
// A Pauli string is two masks of physical index bits as in expect_kernels.h: x = the bits that carry X or Y, z = the
// bits that carry Z or Y, ny = popcount(x & z).  The rotation is R = exp(-i theta P) = cos(theta) I - i sin(theta) P:
// there is NO factor 1/2 on theta (RZ(phi) of the gate table is the rotation of Z by theta = phi / 2).  With
// f = -i sin(theta) i^ny and s(i) = (-1)^popcount(i & z):
//   x == 0:  psi'_j = (cos(theta) + f s(j)) psi_j
//   x != 0:  psi'_j = cos(theta) psi_j + f s(j ^ x) psi_{j ^ x}
// For x != 0 the pair (j, j ^ x), j over the half with the top bit h of x clear, is a 2x2 butterfly: both results come
// from the two old values.
//
// Tile pass (k_rot_tile): the tile walk and the loads of k_expect_tile -- a set T of tile bits (<= 11, the line bits
// 0..2 among them: every global access is a whole 128-byte line), a grid-stride over the tiles -- made
// read-modify-write.  With a tile in LDS the rotations of the pass whose x lies in T are applied one after the other,
// in list order (they do not commute), a __syncthreads() between two of them; the threads share the S/2 pairs of the
// tile (x = 0: its S amplitudes).  z need not lie in T: s(i) = s(inner, z & T) s(outer, z & ~T), and x moves no outer
// bit, so the outer sign is one factor on f per tile and term.  The term loop reads the term table at wave-uniform
// addresses (the loop counter and the tile base are the same in every lane), so these reads are scalar loads.  The
// tile is stored back to the addresses it came from; tiles partition the index space, so the in-place update has no
// hazard between workgroups.  Many rotations per HBM round trip: which count turns the pass from HBM-bound to
// LDS-bound is measured in profiles/r14_rotation_probe.json.
//
// Wide pass (k_rot_wide): one rotation whose x does not fit a tile with the line bits; each lane owns the pairs
// (i, i ^ x) with bit h clear, loads both and stores both.  Correctness, not speed.
struct RotTerm {         // one rotation of a tile pass in tile coordinates (inner bit b <-> physical bit tile_bit[b])
  u64 zo;                // z outside the tile (physical bits): the outer sign
  double c;              // cos(theta)
  double fr, fi;         // f = -i sin(theta) i^ny
  unsigned xi, zi;       // x and z & T compressed onto the tile bits
  int h;                 // the top bit of xi (the pairs run over the half with it clear); -1: x = 0
  int pad_;
};

struct RotArgs {
  double2* amp;
  const RotTerm* terms;
  u64 n_tiles;           // 2^(k - tb)
  u64 outer_mask;        // physical bits outside the tile (outer index bit j <-> the j-th set bit)
  int tile_bit[kExpTileBits];
  int tb;                // tile bits
  int n_terms;           // <= kExpMaxTerms
};

template <bool NT>
__global__ __launch_bounds__(kBlock) void k_rot_tile(const RotArgs a) {
  constexpr int kTile = 1 << kExpTileBits;
  constexpr int kLoads = kTile / kBlock;
  __shared__ double2 tile[kTile];
  const int S = 1 << a.tb;
  const int tid = threadIdx.x;
  // the term table is written before the launch and only read here: read through the constant address space, the
  // loads are scalar (a plain global load after a barrier and next to the stores of the tile stays a vector load)
  typedef __attribute__((address_space(4))) const RotTerm cterm_t;
  cterm_t* const terms = (cterm_t*)(unsigned long long)a.terms;
  u64 off[kLoads];                                  // physical offsets of the amplitudes this thread loads (every tile)
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
      if (tid + it * kBlock < S) x[it] = ld_amp<NT>(a.amp + (base | off[it]));
    // (a thread stores the LDS slots it fills, and every other thread is past the last rotation of the previous tile
    // before that store: no barrier is needed in front of the refill)
#pragma unroll
    for (int it = 0; it < kLoads; ++it)
      if (tid + it * kBlock < S) tile[tid + it * kBlock] = x[it];
    for (int t = 0; t < a.n_terms; ++t) {
      __syncthreads();                              // the tile is filled / rotation t - 1 is done
      RotTerm e;                                    // wave-uniform address: scalar loads (field by field: a struct in
      e.zo = terms[t].zo;                           // another address space has no copy constructor)
      e.c = terms[t].c;
      e.fr = terms[t].fr;
      e.fi = terms[t].fi;
      e.xi = terms[t].xi;
      e.zi = terms[t].zi;
      e.h = terms[t].h;
      const bool neg = __popcll(base & e.zo) & 1;   // the sign over the outer bits: one per tile and term
      const double fr = neg ? -e.fr : e.fr, fi = neg ? -e.fi : e.fi;
      if (e.h < 0) {                                // x = 0: psi_j *= cos + f s(j)
        for (int j = tid; j < S; j += kBlock) {
          const double2 u = tile[j];
          const bool sj = __popc((unsigned)j & e.zi) & 1;
          const double dr = e.c + (sj ? -fr : fr), di = sj ? -fi : fi;
          tile[j] = make_double2(fma(dr, u.x, -(di * u.y)), fma(dr, u.y, di * u.x));
        }
      } else {
        const int low = (1 << e.h) - 1;
        const bool sx = __popc(e.xi & e.zi) & 1;    // s(j ^ x) = s(j) s(x)
        for (int m = tid; m < (S >> 1); m += kBlock) {
          const int j = ((m & ~low) << 1) | (m & low), p = j ^ (int)e.xi;
          const double2 u = tile[j], w = tile[p];
          const bool sj = __popc((unsigned)j & e.zi) & 1;
          // psi'_j = c u + f s(p) w,  psi'_p = c w + f s(j) u
          const double gr = sj ? -fr : fr, gi = sj ? -fi : fi;            // f s(j)
          const double qr = sx ? -gr : gr, qi = sx ? -gi : gi;            // f s(p)
          tile[j] = make_double2(fma(e.c, u.x, fma(qr, w.x, -(qi * w.y))), fma(e.c, u.y, fma(qr, w.y, qi * w.x)));
          tile[p] = make_double2(fma(e.c, w.x, fma(gr, u.x, -(gi * u.y))), fma(e.c, w.y, fma(gr, u.y, gi * u.x)));
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < kLoads; ++it)
      if (tid + it * kBlock < S) st_amp<NT>(a.amp + (base | off[it]), tile[tid + it * kBlock]);
  }
}

struct RotWideArgs {
  double2* amp;
  u64 half;              // amplitudes / 2
  u64 x, z;
  double c, fr, fi;
  int h;
};

template <bool NT>
__global__ __launch_bounds__(kBlock) void k_rot_wide(const RotWideArgs a) {
  const u64 stride = (u64)gridDim.x * kBlock;
  const u64 low = (1ull << a.h) - 1;
  const bool sx = __popcll(a.x & a.z) & 1;
  for (u64 m = (u64)blockIdx.x * kBlock + threadIdx.x; m < a.half; m += stride) {
    const u64 i = ((m & ~low) << 1) | (m & low), p = i ^ a.x;
    const double2 u = ld_amp<NT>(a.amp + i), w = ld_amp<NT>(a.amp + p);
    const bool si = __popcll(i & a.z) & 1;
    const double gr = si ? -a.fr : a.fr, gi = si ? -a.fi : a.fi;          // f s(i)
    const double qr = sx ? -gr : gr, qi = sx ? -gi : gi;                  // f s(p)
    st_amp<NT>(a.amp + i, make_double2(fma(a.c, u.x, fma(qr, w.x, -(qi * w.y))), fma(a.c, u.y, fma(qr, w.y, qi * w.x))));
    st_amp<NT>(a.amp + p, make_double2(fma(a.c, w.x, fma(gr, u.x, -(gi * u.y))), fma(a.c, w.y, fma(gr, u.y, gi * u.x))));
  }
}

// ---- host: the pass plan (pure, no GPU)
// ORDER PRESERVING, because rotations do not commute: the list is walked once.  A rotation whose x and the line bits
// exceed K = min(k, kExpTileBits) bits gets a wide pass of its own (tile mask 0) and closes the open pass; any other
// joins the open pass when that holds fewer than kExpMaxTerms rotations and its tile bits stay within K with x added,
// else it opens a new pass with T = line | x.  Finished tiles are completed to K bits with the lowest free bits, as
// plan_expectation does.  pass_of is non-decreasing.
struct RotPlan {
  std::vector<int32_t> pass_of;   // per rotation
  std::vector<u64> tile;          // per pass (0: wide)
  std::vector<int> count;         // rotations per pass
};

static int plan_rotations(int k, int n, const uint64_t* x, RotPlan* p) {
  if (k < 0 || k > 63) return fail(QSIM_ERR_INVALID, "qsim_plan_pauli_rotations: %d local qubits", k);
  if (n < 0) return fail(QSIM_ERR_INVALID, "qsim_plan_pauli_rotations: n = %d", n);
  if (n > 0 && !x) return fail(QSIM_ERR_INVALID, "qsim_plan_pauli_rotations: null x_masks");
  const u64 all = (1ull << k) - 1;
  for (int t = 0; t < n; ++t)
    if (x[t] & ~all)
      return fail(QSIM_ERR_NONLOCAL, "rotation %d: X/Y on index bit %d >= log2(chunk_size)=%d", t, 63 - __builtin_clzll(x[t] & ~all), k);
  const int K = std::min(k, kExpTileBits);
  const u64 line = (1ull << std::min(k, kExpLineBits)) - 1;
  p->pass_of.assign((size_t)n, -1);
  p->tile.clear();
  p->count.clear();
  bool open = false;                                // the last pass is a tile pass that may still take rotations
  for (int t = 0; t < n; ++t) {
    if (__builtin_popcountll(x[t] | line) > K) {
      p->tile.push_back(0);
      p->count.push_back(0);
      open = false;
    } else if (!open || p->count.back() >= kExpMaxTerms || __builtin_popcountll(p->tile.back() | x[t]) > K) {
      p->tile.push_back(line);
      p->count.push_back(0);
      open = true;
    }
    if (open) p->tile.back() |= x[t];
    ++p->count.back();
    p->pass_of[(size_t)t] = (int32_t)p->tile.size() - 1;
  }
  for (u64& m : p->tile)
    if (m)
      for (int b = 0; b < k && __builtin_popcountll(m) < K; ++b) m |= 1ull << b;
  return QSIM_OK;
}

// (cos(theta), f = -i sin(theta) i^ny) of a rotation, in double on the host: -i i^ny = -i, 1, i, -1 for ny = 0..3
static void rot_factors(u64 x, u64 z, double theta, double* c, double* fr, double* fi) {
  static const double kr[4] = {0.0, 1.0, 0.0, -1.0}, ki[4] = {-1.0, 0.0, 1.0, 0.0};
  const int ny = __builtin_popcountll(x & z) & 3;
  const double s = std::sin(theta);
  *c = std::cos(theta);
  *fr = kr[ny] * s;
  *fi = ki[ny] * s;
}
