// abi_gates.h -- C ABI: gates and op lists on one chunk, the dense block, the partner-chunk pair and quad forms; the
// op-list checks that the planning entry points (abi_plan.h) and qsim_apply_ops_io (abi_relayout.h) share.
// Part of the single translation unit qsim_hip.hip (included there, in order; not a standalone header).

// How check_op_list reports a qubit outside [0, qubit_limit): the chunk forms (check_local_qubit's two errors), the planners
// without a chunk (the non-local text for a negative qubit too), qsim_plan_peek_pass (its limit is the whole state's qubit count).
enum QubitReport { kQubitOfChunk, kQubitOfPlan, kQubitOfState };

// Every op has arity 1 or 2, qubits below the limit and, with two qubits, distinct ones: checked before anything is launched.
static int check_op_list(int n_ops, const int32_t* nq, const int32_t* qubits, const double* mats, int qubit_limit, QubitReport how) {
  if (n_ops < 0 || (n_ops && (!nq || !qubits || !mats))) return fail(QSIM_ERR_INVALID, "bad op list");
  for (int i = 0; i < n_ops; ++i) {
    if (nq[i] != 1 && nq[i] != 2) return fail(QSIM_ERR_INVALID, "op %d: arity %d", i, nq[i]);
    for (int j = 0; j < nq[i]; ++j) {
      const int q = qubits[2 * i + j];
      if (q >= 0 && q < qubit_limit) continue;
      if (how == kQubitOfState) return fail(QSIM_ERR_INVALID, "op %d: qubit %d out of range", i, q);
      if (how == kQubitOfChunk && q < 0) return fail(QSIM_ERR_INVALID, "qubit %d is negative", q);
      return fail(QSIM_ERR_NONLOCAL, "qubit %d >= log2(chunk_size)=%d: non-local gate requires layout/collect step", q, qubit_limit);
    }
    if (nq[i] == 2 && qubits[2 * i] == qubits[2 * i + 1]) return fail(QSIM_ERR_INVALID, "op %d: repeated qubit", i);
  }
  return QSIM_OK;
}

// The op list as the pass builder takes it: identities drop out; origin (optional): classified op -> index in the caller's list.
static void classify_ops(int n_ops, const int32_t* nq, const int32_t* qubits, const double* mats, std::vector<FusedOp>* ops,
                         std::vector<int32_t>* origin = nullptr) {
  ops->reserve((size_t)n_ops);
  for (int i = 0; i < n_ops; ++i) {
    FusedOp o;
    if (!classify_op(nq[i], qubits + 2 * i, mats + 32 * (size_t)i, &o)) continue;
    ops->push_back(o);
    if (origin) origin->push_back(i);
  }
}

static int validate_ops(qsim_chunk* c, int n_ops, const int32_t* nq, const int32_t* qubits, const double* mats) {
  int rc = check_chunk(c, "qsim_apply_ops");
  if (rc) return rc;
  return check_op_list(n_ops, nq, qubits, mats, c->k, kQubitOfChunk);
}

extern "C" {
int qsim_apply_1q(qsim_chunk* c, int qubit, const double U[8]) {
  int rc = check_chunk(c, "qsim_apply_1q");
  if (rc || (rc = check_local_qubit(c, qubit))) return rc;
  if (!U) return fail(QSIM_ERR_INVALID, "U is null");
  HIP_TRY(hipSetDevice(c->device));
  Group g = {{c, nullptr, nullptr, nullptr}, 1, c->k};
  return gate_1q(g, qubit, U, c->stream);
}

int qsim_apply_2q(qsim_chunk* c, int qa, int qb, const double U[32]) {
  int rc = check_chunk(c, "qsim_apply_2q");
  if (rc || (rc = check_local_qubit(c, qa)) || (rc = check_local_qubit(c, qb))) return rc;
  if (qa == qb) return fail(QSIM_ERR_INVALID, "apply_2q needs two distinct qubits, got %d twice", qa);
  if (!U) return fail(QSIM_ERR_INVALID, "U is null");
  HIP_TRY(hipSetDevice(c->device));
  Group g = {{c, nullptr, nullptr, nullptr}, 1, c->k};
  return gate_2q(g, qa, qb, U, c->stream);
}

int qsim_apply_ops_unfused(qsim_chunk* c, int n_ops, const int32_t* nq, const int32_t* qubits, const double* mats) {
  int rc = validate_ops(c, n_ops, nq, qubits, mats);
  if (rc) return rc;
  for (int i = 0; i < n_ops; ++i) {
    rc = nq[i] == 1 ? qsim_apply_1q(c, qubits[2 * i], mats + 32 * (size_t)i)
                    : qsim_apply_2q(c, qubits[2 * i], qubits[2 * i + 1], mats + 32 * (size_t)i);
    if (rc) return rc;
  }
  return QSIM_OK;
}

// qsim_apply_ops and qsim_apply_ops_tiled (n_tiles = 0: the pass builder searches every tile itself)
static int apply_ops_fused(qsim_chunk* c, int n_ops, const int32_t* nq, const int32_t* qubits, const double* mats,
                           int n_tiles, const uint64_t* tile_masks, const char* what, const int32_t* earliest_pass = nullptr) {
  int rc = validate_ops(c, n_ops, nq, qubits, mats);
  if (rc) return rc;
  if (n_tiles < 0 || (n_tiles && !tile_masks)) return fail(QSIM_ERR_INVALID, "%s: bad tile list", what);
  if ((rc = require_no_parts(c, what))) return rc;
  if (n_ops < 2 || c->k < kTileMinChunk || c->k > kTileMaxQubits) {
    c->last_passes = n_ops;
    return qsim_apply_ops_unfused(c, n_ops, nq, qubits, mats);
  }
  HIP_TRY(hipSetDevice(c->device));
  std::vector<FusedOp> ops;
  std::vector<int32_t> origin, placed;           // (identities drop out of the planned list: the placement follows)
  classify_ops(n_ops, nq, qubits, mats, &ops, &origin);
  int passes = 0;
  TileHint hint = {tile_masks, n_tiles};
  if (earliest_pass && n_tiles) {
    for (int32_t i : origin) placed.push_back(earliest_pass[i]);
    hint.earliest = placed.data();
  }
  rc = run_fused(c, ops, RawOps{n_ops, nq, qubits, mats}, n_tiles ? &hint : nullptr, nullptr, &passes,
                 [&](TileArgs& a, int T, double alg_bytes, bool) { return dispatch_planned(c, a, T, alg_bytes); });
  c->last_passes = passes;
  return rc;
}

int qsim_apply_ops(qsim_chunk* c, int n_ops, const int32_t* nq, const int32_t* qubits, const double* mats) {
  return apply_ops_fused(c, n_ops, nq, qubits, mats, 0, nullptr, "qsim_apply_ops");
}
// qsim_apply_ops with the high tile bits of the first n_tiles passes named by the caller (bit b of tile_masks[p]: index bit b
// is a tile bit of pass p): the pass builder takes them instead of searching; a mask that holds no op is ignored.
int qsim_apply_ops_tiled(qsim_chunk* c, int n_ops, const int32_t* nq, const int32_t* qubits, const double* mats,
                         int n_tiles, const uint64_t* tile_masks) {
  return apply_ops_fused(c, n_ops, nq, qubits, mats, n_tiles, tile_masks, "qsim_apply_ops_tiled");
}
// ... and with a placement: op i not before pass earliest_pass[i] of the named passes (TileHint::earliest)
int qsim_apply_ops_placed(qsim_chunk* c, int n_ops, const int32_t* nq, const int32_t* qubits, const double* mats,
                          int n_tiles, const uint64_t* tile_masks, const int32_t* earliest_pass) {
  return apply_ops_fused(c, n_ops, nq, qubits, mats, n_tiles, tile_masks, "qsim_apply_ops_placed", earliest_pass);
}

}  // extern "C"

// ---- cyclic plans (include/qsim_hip.h; the search: tile_search.h plan_search_cycle; the deferred tail: abi_pending.h) ------
struct qsim_cycle {
  int k;
  u64 id;                            // what a chunk's deferred tail names its cycle by
  PassList head, steady, tail;
};
static std::atomic<u64> g_cycle_ids{0};

// the passes of one list of a cycle, prepared like the cached passes of qsim_apply_ops_placed (no buffers yet)
static int cycle_passes(int k, const qsim_cycle_list* l, const char* part, PassList* out) {
  if (!l || l->n_ops < 1 || l->n_tiles < 0 || (l->n_tiles && !l->tile_masks))
    return fail(QSIM_ERR_INVALID, "qsim_cycle_create: bad %s list", part);
  int rc = check_op_list(l->n_ops, l->nq, l->qubits, l->mats, k, kQubitOfPlan);
  if (rc) return rc;
  std::vector<FusedOp> ops;
  std::vector<int32_t> origin, placed;
  classify_ops(l->n_ops, l->nq, l->qubits, l->mats, &ops, &origin);
  if (ops.empty()) return fail(QSIM_ERR_INVALID, "qsim_cycle_create: the %s list holds identities only", part);
  TileHint hint = {l->tile_masks, l->n_tiles};
  if (l->earliest_pass && l->n_tiles) {
    for (int32_t i : origin) placed.push_back(l->earliest_pass[i]);
    hint.earliest = placed.data();
  }
  auto made = std::make_shared<std::vector<CachedPass>>();
  int passes = 0;
  rc = plan_fused(k, ops, &passes, [&](TileArgs& a, int T, double alg_bytes, bool, bool) {
    lower_unit_real(&a);
    made->push_back(CachedPass{a, T, alg_bytes});
    return (int)QSIM_OK;
  }, l->n_tiles ? &hint : nullptr);
  *out = made;
  return rc;
}

extern "C" {
int qsim_cycle_create(int n_local_qubits, const qsim_cycle_list* head, const qsim_cycle_list* steady, const qsim_cycle_list* tail,
                      int32_t* n_passes, qsim_cycle** out) {
  if (!out) return fail(QSIM_ERR_INVALID, "qsim_cycle_create: out is null");
  if (n_local_qubits < kTileMinChunk || n_local_qubits > kTileMaxQubits)
    return fail(QSIM_ERR_INVALID, "qsim_cycle_create: fused passes need %d..%d local qubits", kTileMinChunk, kTileMaxQubits);
  std::unique_ptr<qsim_cycle> cy(new qsim_cycle());
  cy->k = n_local_qubits;
  cy->id = ++g_cycle_ids;
  int rc = cycle_passes(n_local_qubits, head, "head", &cy->head);
  if (rc || (rc = cycle_passes(n_local_qubits, steady, "steady", &cy->steady)) || (rc = cycle_passes(n_local_qubits, tail, "tail", &cy->tail)))
    return rc;
  if (n_passes) { n_passes[0] = (int32_t)cy->head->size(); n_passes[1] = (int32_t)cy->steady->size(); n_passes[2] = (int32_t)cy->tail->size(); }
  *out = cy.release();
  return QSIM_OK;
}

int qsim_cycle_destroy(qsim_cycle* cycle) {
  delete cycle;                      // (a tail deferred on a chunk keeps its passes alive)
  return QSIM_OK;
}

int qsim_apply_cycle(qsim_chunk* c, const qsim_cycle* cycle) {
  int rc = check_chunk_unsettled(c, "qsim_apply_cycle");
  if (rc) return rc;
  if (!cycle) return fail(QSIM_ERR_INVALID, "qsim_apply_cycle: null cycle");
  if (cycle->k != c->k) return fail(QSIM_ERR_INVALID, "qsim_apply_cycle: a cycle for %d qubits on a chunk of %d", cycle->k, c->k);
  if (!c->owns_memory || c->parent)
    return fail(QSIM_ERR_INVALID, "qsim_apply_cycle: the chunk must own its memory (views and wrapped pointers cannot defer a tail)");
  if ((rc = require_no_parts(c, "qsim_apply_cycle"))) return rc;
  const bool steady = c->deferred && c->deferred->passes && c->deferred->id == cycle->id;
  if (!steady && (rc = settle(c))) return rc;
  if (!c->deferred) c->deferred = new DeferredTail();
  c->deferred->passes.reset();       // (steady: the tail runs now, as the front of B.A)
  const std::vector<CachedPass>& run = steady ? *cycle->steady : *cycle->head;
  if ((rc = launch_passes(c, run))) return rc;
  c->deferred->id = cycle->id;
  c->deferred->passes = cycle->tail;
  c->last_passes = (int)run.size();
  return QSIM_OK;
}

// Dense k-qubit block: new[idx with the block's bits = out] = sum_in M[out][in] old[idx with the block's bits = in], pattern
// bit i <-> qubits[i] -- v3's `_apply_combined_matrix` (parallel_gate_applicator.py:315-385) for a genuinely dense 2^k x 2^k
// matrix (its tensor-product blocks are cheaper as butterflies inside a fused pass: qsim_apply_ops).  1 <= k <= 6.
// k = 1, 2: the pair kernels.  k >= 3 on chunks of >= 2^(k+4) amplitudes: the matrix cores (dense_kernels.h k_dense_mfma2: 16
// blocks per wave and step as the columns of v_mfma_f64_16x16x4_f64; the matrix image in registers for k = 3, 4, in LDS for
// k = 5, 6).  Smaller chunks: one workgroup per block through LDS (k_dense_small).
int qsim_apply_fused_k(qsim_chunk* c, int k, const int32_t* qubits, const double* M) {
  int rc = check_chunk(c, "qsim_apply_fused_k");
  if (rc) return rc;
  if (!qubits || !M) return fail(QSIM_ERR_INVALID, "qsim_apply_fused_k: null argument");
  if (k < 1 || k > 6) return fail(QSIM_ERR_INVALID, "qsim_apply_fused_k: 1 <= k <= 6 qubits expected, got %d", k);
  if ((rc = require_no_parts(c, "qsim_apply_fused_k"))) return rc;
  for (int i = 0; i < k; ++i) {
    if ((rc = check_local_qubit(c, qubits[i]))) return rc;
    for (int j = 0; j < i; ++j) if (qubits[j] == qubits[i]) return fail(QSIM_ERR_INVALID, "qsim_apply_fused_k: repeated qubit %d", qubits[i]);
  }
  if (k == 1) return qsim_apply_1q(c, qubits[0], M);
  if (k == 2) return qsim_apply_2q(c, qubits[1], qubits[0], M);   // pattern = bit(q0) + 2 bit(q1) = the pair index with qa = q1
  return apply_dense_block(c, k, qubits, M);
}

int qsim_last_pass_count(const qsim_chunk* c) { return c ? c->last_passes : -1; }

int qsim_apply_1q_pair(qsim_chunk* c0, qsim_chunk* c1, const double U[8]) {
  qsim_chunk* cs[2] = {c0, c1};
  int rc = check_group(cs, 2, "qsim_apply_1q_pair");
  if (rc) return rc;
  if (!U) return fail(QSIM_ERR_INVALID, "U is null");
  HIP_TRY(hipSetDevice(c0->device));
  Group g = {{c0, c1, nullptr, nullptr}, 2, c0->k};
  return gate_1q(g, c0->k, U, c0->stream);
}

// one qubit local, the other the bit that tells c0 from c1 (virtual bit k)
static int apply_2q_pair(qsim_chunk* c0, qsim_chunk* c1, int q_local, bool qa_is_local, const double U[32], const char* what) {
  qsim_chunk* cs[2] = {c0, c1};
  int rc = check_group(cs, 2, what);
  if (rc || (rc = check_local_qubit(c0, q_local))) return rc;
  if (!U) return fail(QSIM_ERR_INVALID, "U is null");
  HIP_TRY(hipSetDevice(c0->device));
  Group g = {{c0, c1, nullptr, nullptr}, 2, c0->k};
  return qa_is_local ? gate_2q(g, q_local, c0->k, U, c0->stream) : gate_2q(g, c0->k, q_local, U, c0->stream);
}
int qsim_apply_2q_pair_qa_local(qsim_chunk* c0, qsim_chunk* c1, int qa, const double U[32]) {
  return apply_2q_pair(c0, c1, qa, true, U, "qsim_apply_2q_pair_qa_local");
}
int qsim_apply_2q_pair_qb_local(qsim_chunk* c0, qsim_chunk* c1, int qb, const double U[32]) {
  return apply_2q_pair(c0, c1, qb, false, U, "qsim_apply_2q_pair_qb_local");
}

int qsim_apply_2q_quad(qsim_chunk* c00, qsim_chunk* c01, qsim_chunk* c10, qsim_chunk* c11, const double U[32]) {
  qsim_chunk* cs[4] = {c00, c01, c10, c11};
  int rc = check_group(cs, 4, "qsim_apply_2q_quad");
  if (rc) return rc;
  if (!U) return fail(QSIM_ERR_INVALID, "U is null");
  HIP_TRY(hipSetDevice(c00->device));
  // chunk index = 2*bit(qa) + bit(qb): qb is virtual bit k, qa is virtual bit k+1
  Group g = {{c00, c01, c10, c11}, 4, c00->k};
  return gate_2q(g, c00->k + 1, c00->k, U, c00->stream);
}
}  // extern "C"
