// rot_kernels.h -- Pauli rotations exp(-i theta P) (qsim_plan_pauli_rotations, qsim_apply_pauli_rotations).
// Part of the single translation unit qsim_hip.hip (included there after expect_kernels.h; not a standalone header).
//
// Masks, ny and s(i) as in pauli_tile.h.  The rotation is R = exp(-i theta P) = cos(theta) I - i sin(theta) P: there is
// NO factor 1/2 on theta (RZ(phi) of the gate table is the rotation of Z by theta = phi / 2).  With
// f = -i sin(theta) i^ny:
//   x == 0:  psi'_j = (cos(theta) + f s(j)) psi_j
//   x != 0:  psi'_j = cos(theta) psi_j + f s(j ^ x) psi_{j ^ x}
// For x != 0 the pair (j, j ^ x), j over the half with the top bit h of x clear, is a 2x2 butterfly: both results come
// from the two old values.
//
// Tile pass (k_rot_tile): the tile walk of pauli_tile.h made read-modify-write.  A term keeps (cos(theta), fr, fi) in
// f0, f1, f2 (kPauliRotation).  With a tile in LDS the rotations of the pass are applied one after the other, in list order
// (they do not commute), a __syncthreads() between two of them; the threads share the S/2 pairs of the tile (x = 0: its
// S amplitudes).  The outer sign is one factor on f per tile and term.  The term loop reads the term table at
// wave-uniform addresses (the loop counter and the tile base are the same in every lane), so these reads are scalar
// loads.  The tile is stored back to the addresses it came from; tiles partition the index space, so the in-place update has no
// hazard between workgroups.  Many rotations per HBM round trip: which count turns the pass from HBM-bound to
// LDS-bound is measured in profiles/r14_rotation_probe.json.
//
// Wide pass (k_rot_wide): one rotation whose x does not fit a tile with the line bits; each lane owns the pairs
// (i, i ^ x) with bit h clear, loads both and stores both.  Correctness, not speed.
struct RotArgs {
  double2* amp;
  const PauliTerm* terms;   // whole records
  TileWalk w;
  int n_terms;           // <= kExpMaxTerms
};

template <bool NT>
__global__ __launch_bounds__(kBlock) void k_rot_tile(const RotArgs a) {
  __shared__ double2 tile[kExpTile];
  const int S = 1 << a.w.tb;
  const int tid = threadIdx.x;
  // the term table is written before the launch and only read here: read through the constant address space, the
  // loads are scalar (a plain global load after a barrier and next to the stores of the tile stays a vector load)
  typedef __attribute__((address_space(4))) const PauliTerm cterm_t;
  cterm_t* const terms = (cterm_t*)(unsigned long long)a.terms;
  u64 off[kExpLoads];
  tile_offsets(a.w, off);
  for (u64 o = blockIdx.x; o < a.w.n_tiles; o += gridDim.x) {
    const u64 base = tile_base(a.w.outer_mask, o);
    double2 x[kExpLoads];
    tile_load<NT>(a.amp, base, off, S, x);
    // (a thread stores the LDS slots it fills, and every other thread is past the last rotation of the previous tile
    // before that store: no barrier is needed in front of the refill)
    tile_fill(tile, S, x);
    for (int t = 0; t < a.n_terms; ++t) {
      __syncthreads();                              // the tile is filled / rotation t - 1 is done
      PauliTerm e;                                  // wave-uniform address: scalar loads (field by field: a struct in
      e.zo = terms[t].zo;                           // another address space has no copy constructor)
      e.f0 = terms[t].f0;
      e.f1 = terms[t].f1;
      e.f2 = terms[t].f2;
      e.xi = terms[t].xi;
      e.zi = terms[t].zi;
      e.h = terms[t].h;
      const bool neg = __popcll(base & e.zo) & 1;   // the sign over the outer bits: one per tile and term
      const double c = e.f0, fr = neg ? -e.f1 : e.f1, fi = neg ? -e.f2 : e.f2;
      if (e.h < 0) {                                // x = 0: psi_j *= cos + f s(j)
        for (int j = tid; j < S; j += kBlock) {
          const double2 u = tile[j];
          const bool sj = __popc((unsigned)j & e.zi) & 1;
          const double dr = c + (sj ? -fr : fr), di = sj ? -fi : fi;
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
          tile[j] = make_double2(fma(c, u.x, fma(qr, w.x, -(qi * w.y))), fma(c, u.y, fma(qr, w.y, qi * w.x)));
          tile[p] = make_double2(fma(c, w.x, fma(gr, u.x, -(gi * u.y))), fma(c, w.y, fma(gr, u.y, gi * u.x)));
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < kExpLoads; ++it)
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
