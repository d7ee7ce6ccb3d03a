// tile_launch.h -- a planned pass on its way to the device: the launch of k_tile, the re-layout fused into the ends of an
// op list, the plan cache and run_fused.  Everything of the fused passes that touches the device lives here.
// Part of the single translation unit qsim_hip.hip (included there, in order; not a standalone header).
// Tile order of a launch (k_tile).  Gate-less passes depend strongly on it (profiles/r02f_tile_order_probe.txt:
// 2.38 -> 1.58 ms for tile bits {3,4,5,6,18,19,20,21} with bit-reversed order, 1.90 -> 1.70 ms averaged over ten
// tile-bit sets with a bits-above-18 rule), but passes that carry their gates do not: per pass the best of the
// three orders is within 2 % of consecutive tiles on the bench circuit (profiles/r02i_pass_times_by_order.txt),
// so the product launches consecutive tiles; the other orders stay reachable in the probe build.
static int tile_order_for(const TileArgs&, int) {
#ifdef QSIM_PROBES
  if (tuning().tile_order >= 0) return tuning().tile_order;
#endif
  return 0;
}

// physical bit of logical index bit b under a slab layout (host mirror of k_tile's slab_base)
static uint8_t slab_position(const TileSlab& t, int b) {
  for (int j = 0; j < 3; ++j) if (t.bit[j] == b) return (uint8_t)(t.top + j);
  for (int i = 0; i < 4; ++i) if ((t.field[i] >> b) & 1) return (uint8_t)(b - i);
  return (uint8_t)b;
}

// ---- probes of a launch (tools/): empty in the product library -------------------------------------------------------
// memory probe (WRONG results): QSIM_DEBUG_OUT_OF_PLACE: tiles are stored into a second buffer
static void probe_out_of_place(TileArgs* args, const qsim_chunk* c) {
#ifdef QSIM_PROBES
  if (getenv("QSIM_DEBUG_OUT_OF_PLACE")) {
    static double2* other = nullptr;
    static size_t other_bytes = 0;
    const size_t need = sizeof(double2) << c->k;
    if (other_bytes < need) { if (other) (void)hipFree(other); (void)hipMalloc((void**)&other, need); other_bytes = need; }
    args->amp_out = other;
  }
#endif
}
// in-kernel stamps: QSIM_DEBUG_STAMPS=<file> dumps entry / loaded / engine / stored cycle stamps of every 64th workgroup
static void probe_stamps_arm(TileArgs* args, u64 ntiles, hipStream_t stream) {
#ifdef QSIM_PROBES
  static unsigned long long* dbuf = nullptr;
  static const char* path = getenv("QSIM_DEBUG_STAMPS");
  if (path && !dbuf) (void)hipMalloc((void**)&dbuf, sizeof(unsigned long long) * 4 * ((1u << 22)));
  unsigned long long* p = path ? dbuf : nullptr;
  std::memcpy(reinterpret_cast<unsigned char*>(args) + kTileArgBytes - 8, &p, 8);
  if (p) (void)hipMemsetAsync(p, 0, sizeof(unsigned long long) * 4 * (ntiles / 64 + 1), stream);
#endif
}
static void probe_stamps_dump(const TileArgs& args, int nrec, u64 ntiles, hipStream_t stream) {
#ifdef QSIM_PROBES
  if (const char* path = getenv("QSIM_DEBUG_STAMPS")) {
    unsigned long long* p = nullptr;
    std::memcpy(&p, reinterpret_cast<const unsigned char*>(&args) + kTileArgBytes - 8, 8);
    std::vector<unsigned long long> host(4 * (ntiles / 64 + 1));
    (void)hipStreamSynchronize(stream);
    (void)hipMemcpy(host.data(), p, host.size() * 8, hipMemcpyDeviceToHost);
    if (FILE* f = std::fopen(path, "a")) {
      std::fprintf(f, "# pass nrec %d ntiles %llu\n", nrec, (u64)ntiles);
      for (size_t i = 0; i + 3 < host.size(); i += 4)
        if (host[i]) std::fprintf(f, "%llu %llu %llu %llu\n", host[i], host[i + 1], host[i + 2], host[i + 3]);
      std::fclose(f);
    }
  }
#endif
}

#ifndef QSIM_TILES_PER_WG
#define QSIM_TILES_PER_WG 2
#endif
// the runtime cache policy and offset width as template arguments of k_tile<T, NT, WIDE, TPW, PART>
template <int T, int TPW, bool PART>
static void launch_k_tile(bool nt, bool wide, unsigned grid, hipStream_t stream, const TileArgs& args) {
  if (nt && wide) hipLaunchKernelGGL((k_tile<T, true, true, TPW, PART>), dim3(grid), dim3(kTileThreads), 0, stream, args);
  else if (nt) hipLaunchKernelGGL((k_tile<T, true, false, TPW, PART>), dim3(grid), dim3(kTileThreads), 0, stream, args);
  else if (wide) hipLaunchKernelGGL((k_tile<T, false, true, TPW, PART>), dim3(grid), dim3(kTileThreads), 0, stream, args);
  else hipLaunchKernelGGL((k_tile<T, false, false, TPW, PART>), dim3(grid), dim3(kTileThreads), 0, stream, args);
}

// Tiles per workgroup of a launch of T-bit tiles over a chunk of k qubits with nfix index bits fixed (a partial launch):
// the launch rule as a pure function (qsim_tiles_per_workgroup), 1 or QSIM_TILES_PER_WG; what launch_tile refuses is an
// error here.  Two tiles per workgroup, the second one's loads in flight while the first is computed on
// (profiles/r02r_ab_prefetch_before_engine.txt: -3.9 % per pass; 4 or 8 tiles per workgroup lose it again,
// profiles/r02z_ab_paired_stores.txt).  Also for the 64-bit-offset form (110 VGPRs: the 32 KiB of LDS admit four
// workgroups per CU, so 128 are there); not for small grids.
static int tiles_per_workgroup(int k, int T, int nfix) {
  if (T > kTileBitsMax || T < kTileThreadBits) return fail(QSIM_ERR_INVALID, "internal: tile size %d not built", T);
  if (k < T) return fail(QSIM_ERR_INVALID, "internal: a %d-bit tile on a chunk of %d qubits", T, k);
  if (nfix < 0 || (nfix && (T != kTileBitsMax || nfix > 3 || k - T < nfix)))
    return fail(QSIM_ERR_INVALID, "internal: partial launch of a %d-bit tile", T);
  if (k - T - nfix >= 32) return fail(QSIM_ERR_INVALID, "internal: too many tiles");
  const u64 ntiles = 1ull << (k - T - nfix);            // (nfix: the tiles of one destination slab of a fused re-layout)
  constexpr int TPW = QSIM_TILES_PER_WG;
  return TPW > 1 && ntiles >= (u64)TPW * 4096 ? TPW : 1;
}

template <int T>
static int launch_tile(const TileArgs& a, const qsim_chunk* c, hipStream_t stream, double alg_bytes) {
  if constexpr (T > kTileBitsMax || T < kTileThreadBits) {
    return fail(QSIM_ERR_INVALID, "internal: tile size %d not built", T);
  } else {
  const int per_wg = tiles_per_workgroup(c->k, T, a.nfix);
  if (per_wg < 0) return per_wg;
  const u64 ntiles = 1ull << (c->k - T - a.nfix);
  TileArgs args = a;
  args.ntiles = (uint32_t)ntiles;
  args.order = (uint8_t)((a.order & ~kTileOrderMask) | (tile_order_for(a, T) & kTileOrderMask));
  args.nbits = (uint8_t)c->k;
  if (!args.amp_out) args.amp_out = args.amp;
  // a pass that reads / writes a re-laid-out buffer: the thread layouts become physical bit positions
  for (int i = 0; i < T - kTileLow; ++i) {
    if (args.perm & kTilePermIn) args.lay_in[i] = slab_position(args.slab_in, args.lay_in[i]);
    if (args.perm & kTilePermOut) args.lay_out[i] = slab_position(args.slab_out, args.lay_out[i]);
  }
  probe_out_of_place(&args, c);
  probe_stamps_arm(&args, ntiles, stream);
  // thread part of an element offset: the first min(5, NH) bits of the load / store layouts: 32-bit addressing when
  // all are < 28
  bool wide = false;
  for (int i = 0; i < kTileThreadBits - kTileLow && i < T - kTileLow; ++i) wide = wide || args.lay_in[i] >= 28 || args.lay_out[i] >= 28;
  bool nt = c->span_bytes > tuning().mall_bytes;       // cache policy by state size (gate_plan.h)
  if (tuning().force_nt >= 0) nt = tuning().force_nt != 0;
  constexpr int TPW = QSIM_TILES_PER_WG;
  const bool two = per_wg > 1;                             // (tiles_per_workgroup: the rule)
  const unsigned grid = (unsigned)(two ? ntiles / TPW : ntiles);
  const bool part = T == kTileBitsMax && args.nfix != 0;   // one destination slab: the PART instantiations (full tiles only)
  {
    ProfileScope prof(kClsTile, alg_bytes, stream, nt, 32.0 * (double)(ntiles << T));
    if constexpr (T == kTileBitsMax) {
      if (part && two) launch_k_tile<T, TPW, true>(nt, wide, grid, stream, args);
      else if (part) launch_k_tile<T, 1, true>(nt, wide, grid, stream, args);
    }
    if (!part && two) launch_k_tile<T, TPW, false>(nt, wide, grid, stream, args);
    else if (!part) launch_k_tile<T, 1, false>(nt, wide, grid, stream, args);
  }
  HIP_TRY(hipGetLastError());
  if (!part) probe_stamps_dump(args, a.nrec, ntiles, stream);
  return QSIM_OK;
  }
}

static int launch_tile_any(const TileArgs& a, int T, const qsim_chunk* c, hipStream_t stream, double alg_bytes) {
  switch (T) {
    case 8: return launch_tile<8>(a, c, stream, alg_bytes);
    case 9: return launch_tile<9>(a, c, stream, alg_bytes);
    case 10: return launch_tile<10>(a, c, stream, alg_bytes);
    case 11: return launch_tile<11>(a, c, stream, alg_bytes);
    case 12: return launch_tile<12>(a, c, stream, alg_bytes);
  }
  return fail(QSIM_ERR_INVALID, "internal: tile size %d", T);
}

// ---- re-layout fused into the first / last pass of an op list (qsim_apply_ops_io) -------------------------------
// Slab layout of an all-to-all re-layout over the local bits `bits` (qsim_pack_all): amplitude i of the chunk sits at
//   d * 2^(k - m) + (i with the m bits removed),   d = sum_j bit(i, bits[j]) << j
// of the buffer, i.e. logical index bit bits[j] is physical bit k - m + j and the others close ranks.
struct SlabLayout {
  int m = 0;
  int bits[3] = {0, 0, 0};
};
static void slab_descriptor(int k, const SlabLayout& L, TileSlab* t) {
  int sorted[3] = {64, 64, 64};
  for (int j = 0; j < L.m; ++j) sorted[j] = L.bits[j];
  std::sort(sorted, sorted + L.m);
  auto below = [](int b) -> u64 { return b >= 64 ? ~0ull : ((1ull << b) - 1); };
  t->field[0] = below(sorted[0]);
  for (int i = 1; i < 4; ++i) {
    const int lo = sorted[i - 1], hi = i < 3 ? sorted[i] : 64;
    t->field[i] = lo >= 64 ? 0 : (below(hi) & ~below(lo + 1));
  }
  for (int j = 0; j < 3; ++j) t->bit[j] = (uint8_t)(j < L.m ? L.bits[j] : 63);
  t->top = (uint8_t)(k - L.m);
  std::memset(t->pad, 0, sizeof t->pad);
}
struct FusedIo {
  const qsim_chunk* src = nullptr;   // first pass reads this buffer (slab layout `in`) instead of the chunk
  SlabLayout in;
  qsim_chunk* dst = nullptr;         // last pass stores into this buffer in slab layout `out` ...
  SlabLayout out;
  qsim_chunk* dst_own = nullptr;     // ... except slab `own_pattern`, which goes to this one (same layout)
  int own_pattern = -1;
  bool parts = false;                // the slab-storing pass is not launched here: it is left pending in the chunk and
                                     // launched slab by slab (qsim_apply_ops_io_part), so each slab's exchange can start early
  bool fused_in = false, fused_out = false;   // results
  bool own_in_chunk = false;         // result: the own slab went into the chunk itself (dst_own == src and ONE pass does it all)
};

// One planned pass on its way to the device: buffers and the re-layout of the op list's ends (prepare_planned), then the
// launch (dispatch_planned) -- or, for the slab-storing pass of a split call, nothing yet (stays_for_parts).
static void prepare_planned(qsim_chunk* c, TileArgs& a, int T, bool first, bool last, FusedIo* io) {
  a.amp = c->amp;
  a.amp_out = c->amp;
  a.amp_out_own = nullptr;
  a.perm = 0;
  if (io && first && io->src) {
    a.amp = io->src->amp;
    a.perm |= kTilePermIn;
    slab_descriptor(c->k, io->in, &a.slab_in);
    io->fused_in = true;
  }
  if (io && last && io->dst) {
    // the slab that stays is chosen per tile from the tile's base: its bits must lie outside the tile
    bool clash = false;
    for (int j = 0; j < T - kTileLow; ++j)
      for (int i = 0; i < io->out.m; ++i) clash = clash || a.h[j] == io->out.bits[i];
    if (!clash || io->own_pattern < 0) {
      a.amp_out = io->dst->amp;
      a.perm |= kTilePermOut;
      slab_descriptor(c->k, io->out, &a.slab_out);
      if (io->own_pattern >= 0) {
        a.perm |= kTileOwnOut;
        a.amp_out_own = io->dst_own->amp;
        if (first && io->src && io->dst_own->amp == io->src->amp) {
          // ONE pass reads the source buffer and stores the slabs, and the caller named the source as the place of the
          // slab that stays (three shard-sized buffers per rank instead of four): a tile of that slab must not overwrite
          // source lines other tiles still read -- it goes into the chunk itself, whose contents nobody needs now
          a.amp_out_own = c->amp;
          io->own_in_chunk = true;
        }
        a.own_mask = a.own_value = 0;
        for (int i = 0; i < io->out.m; ++i) {
          a.own_mask |= 1ull << io->out.bits[i];
          if ((io->own_pattern >> i) & 1) a.own_value |= 1ull << io->out.bits[i];
        }
      }
      io->fused_out = true;
    }
  }
}

// The slab-storing pass of a split call (FusedIo::parts) is not launched with the others: qsim_apply_ops_io_part launches
// it piece by piece (full tiles only: the PART instantiations of k_tile).
static bool stays_for_parts(const FusedIo& io, int T, bool last) {
  return last && io.dst && io.parts && io.fused_out && T == kTileBitsMax;
}

static int dispatch_planned(qsim_chunk* c, TileArgs& a, int T, double alg_bytes) {
  if (tuning().debug_stats < 2) return launch_tile_any(a, T, c, c->stream, alg_bytes);
  // QSIM_DEBUG_STATS=2: time every pass synchronously and print its shape (profiling aid)
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
  (void)hipEventRecord(e0, c->stream);
  const int rc = launch_tile_any(a, T, c, c->stream, alg_bytes);
  (void)hipEventRecord(e1, c->stream);
  (void)hipEventSynchronize(e1);
  float ms = 0;
  (void)hipEventElapsedTime(&ms, e0, e1);
  std::fprintf(stderr, "[qsim] timed pass: %.3f ms, %d records, high bits", ms, a.nrec);
  for (int j = 0; j < T - kTileLow; ++j) std::fprintf(stderr, " %d", a.h[j]);
  std::fprintf(stderr, "\n");
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  return rc;
}

// ---- plan cache ---------------------------------------------------------------------------------------------------
// Runners execute the same op list again and again (a planned circuit repeated, one plan per chunk of a chunked run):
// the pass images of the last few op lists are kept, keyed by the exact bytes of the call (local qubits, arities,
// qubits, matrices), and launched again without planning.  Planning overlaps with the device for large states (the
// images of pass p + 1 are made while pass p runs), so this matters where passes are short: 13 % of a step at 22
// qubits, nothing at 28.  Images are stored without buffers or layouts: those are put in at
// launch time (prepare_planned), so one entry serves every chunk of its size and every re-layout.
struct CachedPass { TileArgs a; int T; double alg_bytes; };
struct CachedPlan {
  int k = 0;
  u64 hash = 0;
  std::vector<unsigned char> key;        // nq | qubits | mats of the call
  std::vector<CachedPass> passes;
};
constexpr size_t kPlanCacheEntries = 8;
constexpr size_t kPlanCacheMaxKeyBytes = 4u << 20;      // longer op lists are planned every time
static std::list<CachedPlan> g_plan_cache;             // most recently used first
static std::mutex g_plan_cache_mu;

struct RawOps { int n; const int32_t* nq; const int32_t* qubits; const double* mats; };    // the op list as the caller gave it

// Every pass of the op list, planned (or taken from the cache) and prepared, goes to `sink(a, T, alg_bytes, last)` -- pass
// p before pass p + 1 is planned, so a sink that launches keeps the device busy while the host plans.
template <class Sink>
static int run_fused(qsim_chunk* c, const std::vector<FusedOp>& ops, const RawOps& raw, const TileHint* hint, FusedIo* io,
                     int* n_passes, Sink&& sink) {
  std::vector<unsigned char> key;
  u64 hash = 0;
  const size_t n_ops = (size_t)raw.n;
  const size_t hint_bytes = hint ? sizeof(uint64_t) * (size_t)hint->n : 0;
  const size_t placed_bytes = hint && hint->earliest ? sizeof(int32_t) * ops.size() : 0;
  const int32_t hint_tag[2] = {hint ? hint->n : -1, placed_bytes != 0};   // (named tiles, placement present: no hint list reads as another)
  const size_t key_bytes = n_ops * (sizeof(int32_t) * 3 + sizeof(double) * 32) + sizeof hint_tag + hint_bytes + placed_bytes;
  const bool cacheable = raw.nq && raw.qubits && raw.mats && raw.n > 0 && key_bytes <= kPlanCacheMaxKeyBytes && tuning().debug_stats == 0 &&
                         tuning().debug_skip_gates == 0;     // (probe passes take their tile bits from the environment at plan time)
  if (cacheable) {
    key.resize(key_bytes);
    unsigned char* w = key.data();
    std::memcpy(w, raw.nq, sizeof(int32_t) * n_ops); w += sizeof(int32_t) * n_ops;
    std::memcpy(w, raw.qubits, sizeof(int32_t) * 2 * n_ops); w += sizeof(int32_t) * 2 * n_ops;
    std::memcpy(w, raw.mats, sizeof(double) * 32 * n_ops); w += sizeof(double) * 32 * n_ops;
    std::memcpy(w, hint_tag, sizeof hint_tag); w += sizeof hint_tag;
    if (hint_bytes) std::memcpy(w, hint->masks, hint_bytes);
    if (placed_bytes) std::memcpy(w + hint_bytes, hint->earliest, placed_bytes);
    hash = fnv1a(key.data(), key.size(), 1469598103934665603ull ^ (u64)c->k);
    std::vector<CachedPass> hit;
    {
      std::lock_guard<std::mutex> lock(g_plan_cache_mu);
      for (auto it = g_plan_cache.begin(); it != g_plan_cache.end(); ++it)
        if (it->hash == hash && it->k == c->k && it->key == key) {
          g_plan_cache.splice(g_plan_cache.begin(), g_plan_cache, it);
          hit = g_plan_cache.front().passes;
          break;
        }
    }
    if (!hit.empty()) {
      for (size_t p = 0; p < hit.size(); ++p) {
        const bool last = p + 1 == hit.size();
        prepare_planned(c, hit[p].a, hit[p].T, p == 0, last, io);
        const int rc = sink(hit[p].a, hit[p].T, hit[p].alg_bytes, last);
        if (rc) return rc;
      }
      *n_passes = (int)hit.size();
      return QSIM_OK;
    }
  }
  std::vector<CachedPass> made;
  const int rc = plan_fused(c->k, ops, n_passes, [&](TileArgs& a, int T, double alg_bytes, bool first, bool last) {
    lower_unit_real(&a);
    if (cacheable) made.push_back(CachedPass{a, T, alg_bytes});      // (before buffers and layouts go in)
    prepare_planned(c, a, T, first, last, io);
    return sink(a, T, alg_bytes, last);
  }, hint);
  if (rc == QSIM_OK && cacheable && !made.empty()) {
    std::lock_guard<std::mutex> lock(g_plan_cache_mu);
    g_plan_cache.emplace_front();
    CachedPlan& e = g_plan_cache.front();
    e.k = c->k; e.hash = hash; e.key.swap(key); e.passes.swap(made);
    while (g_plan_cache.size() > kPlanCacheEntries) g_plan_cache.pop_back();
  }
  return rc;
}
