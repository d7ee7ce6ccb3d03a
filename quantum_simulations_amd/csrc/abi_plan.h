// abi_plan.h -- C ABI: the host-only planning entry points (no device, no chunk): what the pass builder would do with an op
// list, pass counts under several layouts, the layout search, the piece rule of the split form.
// Part of the single translation unit qsim_hip.hip (included there, in order; not a standalone header).
extern "C" {
// Forget the cached pass images (run_fused keeps those of the last few op lists): the next call plans again.  For callers
// that time a COLD call (bench.py `api_path`) or changed their mind about memory.
int qsim_plan_cache_clear(void) {
  std::lock_guard<std::mutex> lock(g_plan_cache_mu);
  g_plan_cache.clear();
  return QSIM_OK;
}

static_assert(sizeof(TileArgs) == QSIM_PASS_IMAGE_BYTES, "pass image = the kernel-argument block of k_tile");

}  // extern "C"
// qsim_plan_ops, qsim_plan_ops_tiled (no placement) and qsim_plan_ops_placed: one body, `what` names the call in its errors
static int plan_ops_images(const char* what, int n_local_qubits, int n_ops, const int32_t* nq, const int32_t* qubits,
                           const double* mats, int n_tiles, const uint64_t* tile_masks, const int32_t* earliest_pass, void* out,
                           uint64_t out_capacity_bytes, int32_t* n_passes) {
  if (n_tiles < 0 || (n_tiles && !tile_masks)) return fail(QSIM_ERR_INVALID, "%s: bad tile list", what);
  if (!n_passes) return fail(QSIM_ERR_INVALID, "%s: n_passes is null", what);
  if (n_local_qubits < kTileMinChunk || n_local_qubits > kTileMaxQubits)
    return fail(QSIM_ERR_INVALID, "%s: fused passes need %d..%d local qubits", what, kTileMinChunk, kTileMaxQubits);
  int rc = check_op_list(n_ops, nq, qubits, mats, n_local_qubits, kQubitOfPlan);
  if (rc) return rc;
  std::vector<FusedOp> ops;
  std::vector<int32_t> origin, placed;
  classify_ops(n_ops, nq, qubits, mats, &ops, &origin);
  int passes = 0;
  char* dst = (char*)out;
  uint64_t used = 0;
  TileHint hint = {tile_masks, n_tiles};
  if (earliest_pass && n_tiles) {
    for (int32_t i : origin) placed.push_back(earliest_pass[i]);
    hint.earliest = placed.data();
  }
  rc = plan_fused(n_local_qubits, ops, &passes, [&](TileArgs& a, int T, double, bool, bool) {
    if (dst) {
      if (used + sizeof(TileArgs) > out_capacity_bytes) return fail(QSIM_ERR_INVALID, "%s: output buffer too small", what);
      std::memcpy(dst + used, &a, sizeof a);
    }
    used += sizeof(TileArgs);
    return (int)QSIM_OK;
  }, n_tiles ? &hint : nullptr);
  *n_passes = passes;
  return rc;
}
extern "C" {
int qsim_plan_ops(int n_local_qubits, int n_ops, const int32_t* nq, const int32_t* qubits, const double* mats,
                  void* out, uint64_t out_capacity_bytes, int32_t* n_passes) {
  return plan_ops_images("qsim_plan_ops", n_local_qubits, n_ops, nq, qubits, mats, 0, nullptr, nullptr, out, out_capacity_bytes, n_passes);
}
int qsim_plan_ops_tiled(int n_local_qubits, int n_ops, const int32_t* nq, const int32_t* qubits, const double* mats,
                        int n_tiles, const uint64_t* tile_masks, void* out, uint64_t out_capacity_bytes, int32_t* n_passes) {
  return plan_ops_images("qsim_plan_ops_tiled", n_local_qubits, n_ops, nq, qubits, mats, n_tiles, tile_masks, nullptr, out,
                         out_capacity_bytes, n_passes);
}
int qsim_plan_ops_placed(int n_local_qubits, int n_ops, const int32_t* nq, const int32_t* qubits, const double* mats,
                         int n_tiles, const uint64_t* tile_masks, const int32_t* earliest_pass, void* out,
                         uint64_t out_capacity_bytes, int32_t* n_passes) {
  return plan_ops_images("qsim_plan_ops_placed", n_local_qubits, n_ops, nq, qubits, mats, n_tiles, tile_masks, earliest_pass, out,
                         out_capacity_bytes, n_passes);
}

// What run_fused does to planned pass images before it launches them (tile_groups.h lower_unit_real): the unconditional real
// 2x2 records of the unit-diagonal family become OPC_UNIT1 and their factors go into a matrix or the OPC_SCALE record of
// the pass.  In place, n_images images of QSIM_PASS_IMAGE_BYTES; *n_rewritten (optional): records rewritten.  Host only.
int qsim_lower_pass_images(void* images, int n_images, int32_t* n_rewritten) {
  if (n_images < 0 || (n_images && !images)) return fail(QSIM_ERR_INVALID, "qsim_lower_pass_images: bad arguments");
  int total = 0;
  for (int i = 0; i < n_images; ++i) {
    TileArgs a;
    std::memcpy(&a, (char*)images + (size_t)i * sizeof a, sizeof a);
    total += lower_unit_real(&a);
    std::memcpy((char*)images + (size_t)i * sizeof a, &a, sizeof a);
  }
  if (n_rewritten) *n_rewritten = total;
  return QSIM_OK;
}

// The searching pass builder (tile_search.h): the tiles of a plan of the op list with as few passes as a beam search of
// width `beam` finds (<= 0: the default width), never more than qsim_plan_ops needs.  out_masks[p] = the high tile bits of
// pass p (capacity out_capacity masks; may be NULL to count only); handed to qsim_plan_ops_tiled / qsim_apply_ops_tiled
// they give exactly *n_passes passes.  Host only, no device.
int qsim_plan_search(int n_local_qubits, int n_ops, const int32_t* nq, const int32_t* qubits, const double* mats, int beam,
                     uint64_t* out_masks, int out_capacity, int32_t* n_passes) {
  if (!n_passes || out_capacity < 0) return fail(QSIM_ERR_INVALID, "qsim_plan_search: bad arguments");
  if (n_local_qubits < kTileMinChunk || n_local_qubits > kTileMaxQubits)
    return fail(QSIM_ERR_INVALID, "qsim_plan_search: fused passes need %d..%d local qubits", kTileMinChunk, kTileMaxQubits);
  int rc = check_op_list(n_ops, nq, qubits, mats, n_local_qubits, kQubitOfPlan);
  if (rc) return rc;
#ifdef QSIM_PROBES
  if (beam <= 0) if (const char* e = getenv("QSIM_PLAN_BEAM")) beam = atoi(e);
#endif
  // (the one-triple case of qsim_plan_search_triples: the qubits that are on the line bits stay there, nothing bounds it)
  ListSearch ts;
  ts.beam = beam;
  ts.bounded = false;
  rc = plan_search_triples(n_local_qubits, n_ops, nq, qubits, mats, {LineTriple{{0, 1, 2}}}, &ts);
  if (rc) return rc;
  const std::vector<u64>& masks = ts.masks[0];
  *n_passes = ts.best;
  if (out_masks) {
    if ((int)masks.size() > out_capacity) return fail(QSIM_ERR_INVALID, "qsim_plan_search: output buffer too small");
    for (size_t p = 0; p < masks.size(); ++p) out_masks[p] = masks[p];
  }
  return QSIM_OK;
}

// qsim_plan_search of ONE op list under many line-qubit triples (tile_search.h plan_search_triples): triples[3 t + b] = the
// logical qubit that goes to index bit b under triple t, the qubit that was there taking its place -- the layout
// runner/layout_search.py gives a candidate; n_triples = 0: every a < b < c of the n_local_qubits, ascending.  The searches
// run on n_threads host threads (1..64) and share the fewest passes found so far, which ends every search that can no longer
// reach it (flags & QSIM_TRIPLES_UNBOUNDED: none is ended; QSIM_TRIPLES_NEED_BITS: the bound also counts the tile bits a
// state's remaining ops need).  Out: *best_passes, the fewest passes over the triples, and every triple that reaches them,
// sorted by its three qubits (then by position in the list): found_index (position in the list), found_triples (3 each),
// found_masks (*best_passes each, on the triple's index bits: what qsim_plan_search returns for the relabelled list); the
// first two hold one entry per triple searched, found_masks mask_capacity masks -- too few is an error after *best_passes
// and *n_found are written.  histogram (optional, QSIM_PLAN_HISTOGRAM_BINS counts): triples by pass count, the last bin but
// one also holding everything above it, the last bin the searches that were ended (exact counts above the fewest exist
// only unbounded).  The result does not depend on n_threads or on the bound.  Host only, no device.
int qsim_plan_search_triples(int n_local_qubits, int n_ops, const int32_t* nq, const int32_t* qubits, const double* mats,
                             int n_triples, const int32_t* triples, int beam, int n_threads, int flags, int32_t* best_passes,
                             int32_t* n_found, int32_t* found_index, int32_t* found_triples, uint64_t* found_masks,
                             uint64_t mask_capacity, int32_t* histogram) {
  if (!best_passes || !n_found || !found_index || !found_triples || n_triples < 0 || (n_triples && !triples) || (mask_capacity && !found_masks))
    return fail(QSIM_ERR_INVALID, "qsim_plan_search_triples: bad arguments");
  if (n_local_qubits < kTileMinChunk || n_local_qubits > kTileMaxQubits)
    return fail(QSIM_ERR_INVALID, "qsim_plan_search_triples: fused passes need %d..%d local qubits", kTileMinChunk, kTileMaxQubits);
  int rc = check_op_list(n_ops, nq, qubits, mats, n_local_qubits, kQubitOfPlan);
  if (rc) return rc;
  std::vector<LineTriple> list;
  for (int t = 0; t < n_triples; ++t) {
    const int32_t* q = triples + 3 * (size_t)t;
    for (int b = 0; b < 3; ++b)
      if (q[b] < 0 || q[b] >= n_local_qubits || (b && q[b] == q[0]) || (b == 2 && q[2] == q[1]))
        return fail(QSIM_ERR_INVALID, "qsim_plan_search_triples: triple %d is not three qubits of the %d", t, n_local_qubits);
    list.push_back(LineTriple{{q[0], q[1], q[2]}});
  }
  if (!n_triples)
    for (int a = 0; a < n_local_qubits; ++a)
      for (int b = a + 1; b < n_local_qubits; ++b)
        for (int c = b + 1; c < n_local_qubits; ++c) list.push_back(LineTriple{{a, b, c}});
  ListSearch ts;
  ts.beam = beam;
  ts.n_threads = n_threads;
  ts.bounded = !(flags & QSIM_TRIPLES_UNBOUNDED);
  ts.need_bits = (flags & QSIM_TRIPLES_NEED_BITS) != 0;
  rc = plan_search_triples(n_local_qubits, n_ops, nq, qubits, mats, list, &ts);
  if (rc) return rc;
  std::vector<int32_t> found;
  for (size_t t = 0; t < list.size(); ++t) if (ts.passes[t] == ts.best) found.push_back((int32_t)t);
  std::stable_sort(found.begin(), found.end(), [&](int32_t x, int32_t y) {
    return std::lexicographical_compare(list[(size_t)x].q, list[(size_t)x].q + 3, list[(size_t)y].q, list[(size_t)y].q + 3);
  });
  *best_passes = ts.best;
  *n_found = (int32_t)found.size();
  if (histogram) {
    for (int b = 0; b < QSIM_PLAN_HISTOGRAM_BINS; ++b) histogram[b] = 0;
    for (int32_t p : ts.passes) ++histogram[p < 0 ? QSIM_PLAN_HISTOGRAM_BINS - 1 : std::min((int)p, QSIM_PLAN_HISTOGRAM_BINS - 2)];
  }
  if ((uint64_t)found.size() * (uint64_t)ts.best > mask_capacity)
    return fail(QSIM_ERR_INVALID, "qsim_plan_search_triples: output buffer too small (%d triples of %d masks)", (int)found.size(), ts.best);
  for (size_t f = 0; f < found.size(); ++f) {
    const size_t t = (size_t)found[f];
    found_index[f] = found[f];
    for (int b = 0; b < 3; ++b) found_triples[3 * f + b] = list[t].q[b];
    for (int p = 0; p < ts.best; ++p) found_masks[f * (size_t)ts.best + p] = ts.masks[t][(size_t)p];
  }
  return QSIM_OK;
}

// Cyclic plans of ONE op list L that is executed again and again (tile_search.h plan_search_cycle), under the line-qubit
// triples given (as in qsim_plan_search_triples; at least one): L.L is searched under every triple, its tiles replayed for
// the pass of every op, L cut at the first pass that holds an op of the second copy into a head A and a tail B, and A, B.A
// and B searched under the same triple.  R executions are then A (B.A)^(R-1) B.  plain_passes (optional, one per triple):
// the passes of L under the triple where the caller has searched it already; NULL: searched here.  Out, for the triples with
// the fewest steady passes among those whose steady passes are fewer than the plain ones, in list order: found_index,
// found_triples (3 each), found_passes (4 each: plain, head, steady, tail), found_tail (n_ops bytes each: 1 = the op belongs to
// B; inside A and B the ops keep the order of L), found_masks (head, steady and tail tiles one after the other, on the
// triple's index bits) -- one entry per triple given has room for everything but the masks, mask_capacity says how many of
// those fit; too few is an error after *n_found is written.  *n_found = 0, no cycle, is a result and not an error.  The result does
// not depend on n_threads.  Host only, no device.
int qsim_plan_search_cycle(int n_local_qubits, int n_ops, const int32_t* nq, const int32_t* qubits, const double* mats,
                           int n_triples, const int32_t* triples, const int32_t* plain_passes, int beam, int n_threads,
                           int32_t* n_found, int32_t* found_index, int32_t* found_triples, int32_t* found_passes,
                           uint8_t* found_tail, uint64_t* found_masks, uint64_t mask_capacity) {
  if (!n_found || !found_index || !found_triples || !found_passes || !found_tail || n_triples < 1 || !triples || (mask_capacity && !found_masks))
    return fail(QSIM_ERR_INVALID, "qsim_plan_search_cycle: bad arguments");
  if (n_local_qubits < kTileMinChunk || n_local_qubits > kTileMaxQubits)
    return fail(QSIM_ERR_INVALID, "qsim_plan_search_cycle: fused passes need %d..%d local qubits", kTileMinChunk, kTileMaxQubits);
  int rc = check_op_list(n_ops, nq, qubits, mats, n_local_qubits, kQubitOfPlan);
  if (rc) return rc;
  std::vector<LineTriple> list;
  for (int t = 0; t < n_triples; ++t) {
    const int32_t* q = triples + 3 * (size_t)t;
    for (int b = 0; b < 3; ++b)
      if (q[b] < 0 || q[b] >= n_local_qubits || (b && q[b] == q[0]) || (b == 2 && q[2] == q[1]))
        return fail(QSIM_ERR_INVALID, "qsim_plan_search_cycle: triple %d is not three qubits of the %d", t, n_local_qubits);
    list.push_back(LineTriple{{q[0], q[1], q[2]}});
  }
  std::vector<CyclePlan> cycles;
  if ((rc = plan_search_cycle(n_local_qubits, n_ops, nq, qubits, mats, list, plain_passes, beam, n_threads, &cycles))) return rc;
  int fewest = 1 << 30;
  for (const CyclePlan& c : cycles) if (c.found) fewest = std::min(fewest, (int)c.passes[1]);
  int found = 0;
  uint64_t used = 0;
  for (const CyclePlan& c : cycles) if (c.found && c.passes[1] == fewest) { ++found; used += c.masks[0].size() + c.masks[1].size() + c.masks[2].size(); }
  *n_found = found;
  if (used > mask_capacity) return fail(QSIM_ERR_INVALID, "qsim_plan_search_cycle: output buffer too small (%llu masks)", (u64)used);
  size_t f = 0;
  for (size_t t = 0; t < cycles.size(); ++t) {
    const CyclePlan& c = cycles[t];
    if (!c.found || c.passes[1] != fewest) continue;
    found_index[f] = (int32_t)t;
    for (int b = 0; b < 3; ++b) found_triples[3 * f + b] = list[t].q[b];
    found_passes[4 * f] = c.plain;
    for (int w = 0; w < 3; ++w) {
      found_passes[4 * f + 1 + w] = c.passes[w];
      for (u64 m : c.masks[w]) *found_masks++ = m;
    }
    std::memcpy(found_tail + f * (size_t)n_ops, c.tail.data(), (size_t)n_ops);
    ++f;
  }
  return QSIM_OK;
}

// The placement of an op list over its named passes under the caller's prices (tile_search.h plan_balance); earliest_pass
// NULL: the passes are only priced (engine_us_before), nothing is placed.
int qsim_plan_balance(int n_local_qubits, int n_ops, const int32_t* nq, const int32_t* qubits, const double* mats,
                      int n_tiles, const uint64_t* tile_masks, const double* pass_memory_us, const double* engine_costs,
                      int n_engine_costs, int32_t* earliest_pass, double* engine_us_before, double* engine_us_after) {
  if (n_tiles < 1 || !tile_masks || !pass_memory_us) return fail(QSIM_ERR_INVALID, "qsim_plan_balance: bad arguments");
  if (n_local_qubits < kTileMinChunk || n_local_qubits > kTileMaxQubits)
    return fail(QSIM_ERR_INVALID, "qsim_plan_balance: fused passes need %d..%d local qubits", kTileMinChunk, kTileMaxQubits);
  EngineCosts ec;
  if (!engine_costs_from(engine_costs, n_engine_costs, &ec))
    return fail(QSIM_ERR_INVALID, "qsim_plan_balance: the cost table needs %d entries", (int)QSIM_ENGINE_COST_COUNT);
  int rc = check_op_list(n_ops, nq, qubits, mats, n_local_qubits, kQubitOfPlan);
  if (rc) return rc;
  std::vector<FusedOp> ops;
  std::vector<int32_t> origin;
  classify_ops(n_ops, nq, qubits, mats, &ops, &origin);
  const std::vector<u64> masks(tile_masks, tile_masks + n_tiles);
  std::vector<int32_t> placed;
  std::vector<double> before, after;
  rc = plan_balance(n_local_qubits, ops, masks, pass_memory_us, ec, earliest_pass != nullptr, &placed, &before, &after);
  if (rc) return rc;
  for (int i = 0; earliest_pass && i < n_ops; ++i) earliest_pass[i] = 0;
  for (size_t j = 0; earliest_pass && j < origin.size(); ++j) earliest_pass[origin[j]] = placed[j];
  for (int p = 0; p < n_tiles; ++p) {
    if (engine_us_before) engine_us_before[p] = before[(size_t)p];
    if (engine_us_after) engine_us_after[p] = after[(size_t)p];
  }
  return QSIM_OK;
}

// The op list a plan for repeated execution is made from (op_rewrite.h): X / Y gates pushed into their neighbours, CNOTs with
// an exact H on the target turned into CZ.  Same packed format in and out, same amplitudes (up to the rounding of the 2x2
// products); identities drop out.  out_capacity: ops the three output arrays have room for (2 * n_ops + n_qubits is always
// enough); too small a buffer is an error and nothing is written.  need_tile (optional, two counts): the ops that need
// their target inside the tile, before and after.  Host only, no device, deterministic, linear in n_ops.
int qsim_rewrite_ops(int n_qubits, int n_ops, const int32_t* nq, const int32_t* qubits, const double* mats, int32_t* out_nq,
                     int32_t* out_qubits, double* out_mats, int out_capacity, int32_t* n_out, int32_t* need_tile) {
  return qsim_rewrite_ops_priced(n_qubits, n_ops, nq, qubits, mats, out_nq, out_qubits, out_mats, out_capacity, n_out, need_tile, nullptr, 0);
}

// ... with rule (d) of op_rewrite.h under the caller's engine cost table (QSIM_ENGINE_COST_*; NULL: qsim_rewrite_ops).
int qsim_rewrite_ops_priced(int n_qubits, int n_ops, const int32_t* nq, const int32_t* qubits, const double* mats,
                            int32_t* out_nq, int32_t* out_qubits, double* out_mats, int out_capacity, int32_t* n_out,
                            int32_t* need_tile, const double* engine_costs, int n_engine_costs) {
  if (!n_out || out_capacity < 0 || (out_capacity && (!out_nq || !out_qubits || !out_mats)))
    return fail(QSIM_ERR_INVALID, "qsim_rewrite_ops: bad arguments");
  if (n_qubits < 1 || n_qubits > 63) return fail(QSIM_ERR_INVALID, "qsim_rewrite_ops: bad qubit count %d", n_qubits);
  int rc = check_op_list(n_ops, nq, qubits, mats, n_qubits, kQubitOfState);
  if (rc) return rc;
  std::vector<RwOp> ops;
  int need_in = 0, need_out = 0;
  EngineCosts ec;
  const bool priced = engine_costs_from(engine_costs, n_engine_costs, &ec);
  if (engine_costs && !priced) return fail(QSIM_ERR_INVALID, "qsim_rewrite_ops_priced: the cost table has %d entries, not %d", n_engine_costs, (int)QSIM_ENGINE_COST_COUNT);
  rewrite_op_list(n_qubits, n_ops, nq, qubits, mats, &ops, &need_in, priced ? &ec : nullptr);
  *n_out = (int32_t)ops.size();
  if (ops.size() > (size_t)out_capacity) return fail(QSIM_ERR_INVALID, "qsim_rewrite_ops: output buffer too small (%d ops)", (int)ops.size());
  for (size_t i = 0; i < ops.size(); ++i) {
    out_nq[i] = ops[i].nq;
    out_qubits[2 * i] = ops[i].q[0];
    out_qubits[2 * i + 1] = ops[i].nq == 2 ? ops[i].q[1] : 0;
    std::memcpy(out_mats + 32 * i, ops[i].U, sizeof ops[i].U);
    need_out += rw_needs_tile(ops[i]);
  }
  if (need_tile) { need_tile[0] = need_in; need_tile[1] = need_out; }
  return QSIM_OK;
}

// The NEXT fused pass of a partly executed op list on a partitioned state (the partition planner's view of the pass builder,
// runner/partition_plan.py): qubits are index bits of the WHOLE state, the bits >= n_local_qubits are rank bits -- an op may
// use them as controls or phase bits (the rank applies or skips it by its own bits) but an op that TARGETS one has to wait
// for a re-layout and blocks what depends on it.  done[i] != 0: op i ran already.  Out: the high tile bits the pass builder
// would choose now (tile_mask, filled to a whole tile; need_mask: the ones its ops need), and the ops it would hold
// (members, ascending; capacity n_ops).  avoid_mask: bits the fill should leave out (slab bits of the re-layout that follows).
// hint_mask != 0: that tile instead of a searched one.  An empty pass (everything waits for a rank bit) is reported as
// *n_members = 0.  Host only, no device.
int qsim_plan_peek_pass(int n_local_qubits, int n_total_qubits, int n_ops, const int32_t* nq, const int32_t* qubits,
                        const double* mats, const uint8_t* done, uint64_t avoid_mask, uint64_t hint_mask, uint64_t* tile_mask,
                        uint64_t* need_mask, int32_t* n_members, int32_t* members) {
  if (!done || !tile_mask || !n_members || !members) return fail(QSIM_ERR_INVALID, "qsim_plan_peek_pass: null argument");
  if (n_local_qubits < kTileMinChunk || n_local_qubits > kTileMaxQubits)
    return fail(QSIM_ERR_INVALID, "qsim_plan_peek_pass: fused passes need %d..%d local qubits", kTileMinChunk, kTileMaxQubits);
  if (n_total_qubits < n_local_qubits || n_total_qubits > 63) return fail(QSIM_ERR_INVALID, "qsim_plan_peek_pass: bad total qubit count %d", n_total_qubits);
  int rc = check_op_list(n_ops, nq, qubits, mats, n_total_qubits, kQubitOfState);
  if (rc) return rc;
  std::vector<FusedOp> ops;
  std::vector<int32_t> origin;                 // classified op -> index in the caller's list (identities drop out)
  classify_ops(n_ops, nq, qubits, mats, &ops, &origin);
  std::vector<uint8_t> done_ops;
  for (int32_t i : origin) done_ops.push_back(done[i]);
  std::vector<size_t> held;
  PeekPlan peek;
  peek.n_total = n_total_qubits;
  peek.done = done_ops.data();
  peek.avoid = avoid_mask;
  peek.tile_mask = peek.need_mask = 0;
  peek.members = &held;
  int passes = 0;
  const TileHint hint = {&hint_mask, 1};
  rc = plan_fused(n_local_qubits, ops, &passes, [](TileArgs&, int, double, bool, bool) { return (int)QSIM_OK; },
                  hint_mask ? &hint : nullptr, &peek);
  if (rc) return rc;
  *tile_mask = peek.tile_mask;
  if (need_mask) *need_mask = peek.need_mask;
  *n_members = (int32_t)held.size();
  for (size_t j = 0; j < held.size(); ++j) members[j] = origin[held[j]];
  return QSIM_OK;
}

// Pass counts of ONE op list under several qubit layouts (layouts[l * n_local_qubits + q] = the index bit of logical qubit q
// in layout l), planned in parallel on the host: the greedy pass builder's result depends on which three qubits live on the
// line bits (they belong to every tile) -- 17 to 20 passes for the 28-qubit bench circuit -- so an engine that is free to
// choose the layout (runner/engine.py) tries a few dozen and keeps the cheapest.  No device involved.
int qsim_plan_count_layouts(int n_local_qubits, int n_ops, const int32_t* nq, const int32_t* qubits, const double* mats,
                            int n_layouts, const int32_t* layouts, int32_t* n_passes, int n_threads) {
  if (!n_passes || n_layouts < 0 || (n_layouts && !layouts)) return fail(QSIM_ERR_INVALID, "qsim_plan_count_layouts: bad arguments");
  if (n_local_qubits < kTileMinChunk || n_local_qubits > kTileMaxQubits)
    return fail(QSIM_ERR_INVALID, "qsim_plan_count_layouts: fused passes need %d..%d local qubits", kTileMinChunk, kTileMaxQubits);
  const int bad_ops = check_op_list(n_ops, nq, qubits, mats, n_local_qubits, kQubitOfPlan);
  if (bad_ops) return bad_ops;
  for (int l = 0; l < n_layouts; ++l) {
    u64 seen = 0;
    for (int q = 0; q < n_local_qubits; ++q) {
      const int b = layouts[(size_t)l * n_local_qubits + q];
      if (b < 0 || b >= n_local_qubits || ((seen >> b) & 1)) return fail(QSIM_ERR_INVALID, "qsim_plan_count_layouts: layout %d is not a permutation", l);
      seen |= 1ull << b;
    }
  }
  (void)tuning();                                          // (initialised before the threads start)
  std::atomic<int> next{0}, bad{0};
  auto work = [&]() {
    std::vector<FusedOp> ops;
    for (;;) {
      const int l = next.fetch_add(1);
      if (l >= n_layouts) return;
      const int32_t* lay = layouts + (size_t)l * n_local_qubits;
      ops.clear();
      for (int i = 0; i < n_ops; ++i) {
        const int32_t q[2] = {lay[qubits[2 * i]], nq[i] == 2 ? lay[qubits[2 * i + 1]] : -1};
        FusedOp o;
        if (classify_op(nq[i], q, mats + 32 * (size_t)i, &o)) ops.push_back(o);
      }
      int passes = 0;
      const int rc = plan_fused(n_local_qubits, ops, &passes, [](TileArgs&, int, double, bool, bool) { return (int)QSIM_OK; });
      if (rc) bad.store(1);
      n_passes[l] = rc ? -1 : passes;
    }
  };
  const int nt = std::max(1, std::min(n_threads > 0 ? n_threads : 1, std::min(n_layouts, 64)));
  std::vector<std::thread> pool;
  for (int t = 1; t < nt; ++t) pool.emplace_back(work);
  work();
  for (std::thread& t : pool) t.join();
  if (bad.load()) return fail(QSIM_ERR_INVALID, "qsim_plan_count_layouts: a layout could not be planned");
  return QSIM_OK;
}

// Which index bit should every qubit live on so that the tiles of the given passes fall on index-bit sets with a good DRAM
// pattern?  Simulated annealing over the assignment (bits 0..2, the 128-byte line, stay) under the caller's cost model of
// a tile-bit set: c0 + sum_b bit_cost[b - 3] + sum_{a < b} pair_cost[(a - 3) * nb + (b - 3)], nb = top_bit - 2, bits above
// top_bit priced like top_bit (runner/tile_layout.py holds the coefficients: ridge fits to measured passes).  tile_masks[p] =
// the high tile bits of pass p as LOGICAL qubits; out_l2p[q] = the index bit chosen for qubit q.  Host only.
int qsim_choose_layout(int n_local_qubits, int n_tiles, const uint64_t* tile_masks, int top_bit, const double* bit_cost,
                       const double* pair_cost, const double* triple_cost, uint64_t seed, int sweeps, int32_t* out_l2p,
                       double* cost_identity, double* cost_chosen) {
  const int n = n_local_qubits, low = kTileLow;
  if (n < low + 2 || n > 62 || n_tiles < 0 || (n_tiles && !tile_masks) || !bit_cost || !pair_cost || !out_l2p || top_bit < low || top_bit > 62 || sweeps < 1)
    return fail(QSIM_ERR_INVALID, "qsim_choose_layout: bad arguments");
  const int nb = top_bit - low + 1;
  std::vector<std::vector<int>> tiles((size_t)n_tiles);
  std::vector<std::vector<int>> member((size_t)n);
  for (int t = 0; t < n_tiles; ++t)
    for (int q = low; q < n; ++q)
      if ((tile_masks[t] >> q) & 1) { tiles[(size_t)t].push_back(q); member[(size_t)q].push_back(t); }
  std::vector<double> sym((size_t)nb * nb, 0.0);
  for (int a = 0; a < nb; ++a)
    for (int b = a + 1; b < nb; ++b) sym[(size_t)a * nb + b] = sym[(size_t)b * nb + a] = pair_cost[(size_t)a * nb + b];
  std::vector<int> l2p((size_t)n);
  for (int q = 0; q < n; ++q) l2p[(size_t)q] = q;
  // (optional third-order terms: triple_cost[(a * nb + b) * nb + c] for a < b < c, zero elsewhere)
  auto cost_of = [&](int t) {
    int idx[64], m = 0;
    for (int q : tiles[(size_t)t]) idx[m++] = std::min(l2p[(size_t)q], top_bit) - low;
    double c = 0;
    for (int i = 0; i < m; ++i) {
      c += bit_cost[idx[i]];
      for (int j = i + 1; j < m; ++j) c += sym[(size_t)idx[i] * nb + idx[j]];
    }
    if (triple_cost) {
      std::sort(idx, idx + m);
      for (int i = 0; i < m; ++i)
        for (int j = i + 1; j < m; ++j) {
          if (idx[j] == idx[i]) continue;
          const double* row = triple_cost + ((size_t)idx[i] * nb + idx[j]) * nb;
          for (int l = j + 1; l < m; ++l) if (idx[l] != idx[j]) c += row[idx[l]];
        }
    }
    return c;
  };
  std::vector<double> costs((size_t)n_tiles);
  double cur = 0;
  for (int t = 0; t < n_tiles; ++t) cur += (costs[(size_t)t] = cost_of(t));
  const double identity = cur;
  double best = cur;
  std::vector<int> best_l2p = l2p;
  u64 rs = seed * 0x9E3779B97F4A7C15ull + 0x2545F4914F6CDD1Dull;
  auto rnd = [&]() { rs ^= rs << 13; rs ^= rs >> 7; rs ^= rs << 17; return rs; };
  const int np_ = n - low;
  const long steps = (long)sweeps * np_ * np_ / 2;
  const double T0 = std::max(1e-3, 0.03 * identity / std::max(1, n_tiles));
  std::vector<int> touched;
  std::vector<double> fresh;
  for (long it = 0; it < steps && n_tiles > 0; ++it) {
    const int a = low + (int)(rnd() % (u64)np_);
    int b = low + (int)(rnd() % (u64)(np_ - 1));
    if (b >= a) ++b;
    touched.clear();
    for (int t : member[(size_t)a]) touched.push_back(t);
    for (int t : member[(size_t)b]) if (std::find(touched.begin(), touched.end(), t) == touched.end()) touched.push_back(t);
    if (touched.empty()) continue;
    std::swap(l2p[(size_t)a], l2p[(size_t)b]);
    fresh.clear();
    double delta = 0;
    for (int t : touched) { fresh.push_back(cost_of(t)); delta += fresh.back() - costs[(size_t)t]; }
    const double T = T0 * (1.0 - (double)it / (double)steps) + 1e-4;
    const double u = (double)(rnd() >> 11) * 0x1p-53;
    if (delta < 0 || u < std::exp(-delta / T)) {
      for (size_t i = 0; i < touched.size(); ++i) costs[(size_t)touched[i]] = fresh[i];
      cur += delta;
      if (cur < best - 1e-12) { best = cur; best_l2p = l2p; }
    } else {
      std::swap(l2p[(size_t)a], l2p[(size_t)b]);
    }
  }
  for (int q = 0; q < n; ++q) out_l2p[q] = best_l2p[(size_t)q];
  if (cost_identity) *cost_identity = identity;
  if (cost_chosen) *cost_chosen = best;
  return QSIM_OK;
}

// (k, m, pieces asked for) -> pieces made: the rule of the split form as a pure function (schedulers, dry runs, tests)
int qsim_split_piece_count(int n_local_qubits, int m, int dst_parts) {
  if (m < 1 || m > 3 || m > n_local_qubits || dst_parts == 0) return 1;
  return PieceCut::cut(n_local_qubits, m, nullptr, dst_parts).n_parts();
}

// (k, T, fixed bits of a partial launch) -> tiles one workgroup of the fused pass takes: launch_tile's own rule
int qsim_tiles_per_workgroup(int n_local_qubits, int tile_bits, int n_fixed_bits) {
  return tiles_per_workgroup(n_local_qubits, tile_bits, n_fixed_bits);
}
}  // extern "C"
