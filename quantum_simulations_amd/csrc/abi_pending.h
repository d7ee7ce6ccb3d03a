// abi_pending.h -- what a split qsim_apply_ops_io call (abi_relayout.h) leaves pending on a chunk; every topic of the C ABI asks.
// Part of the single translation unit qsim_hip.hip (included there, in order; not a standalone header).

// An op list whose SOURCE arrives in pieces (qsim_ops_io::src_parts: the receive side of a fused re-layout): planned and
// prepared at the call, launched as the pieces are announced (qsim_apply_ops_io_load) -- the first pass as partial launches
// over the tiles whose source pieces are there, the rest when the source is complete.
struct DeferredIo {
  bool active = false;
  bool tiles = false;               // tile passes (else: chunk too small / no ops: gate by gate after the source is complete)
  int n_ops = 0;
  std::vector<int32_t> nq, qubits;  // the op list (kept for the gate-by-gate case)
  std::vector<double> mats;
  qsim_ops_io io;
  FusedIo fio;
  std::vector<CachedPass> passes;   // prepared passes (buffers in)
  int nb = 0;                       // 2^nb source pieces: the top nb index bits that are no source slab bits
  int piece_bit[3] = {0, 0, 0};     // ascending
  int nb_free = 0;                  // the first pass runs as 2^nb_free partial launches (0: whole, after the last piece)
  unsigned announced = 0, launched = 0;
};

static bool parts_pending(const qsim_chunk* c) {
  return (c->pending && c->pending->mode != PendingLast::kNone) || (c->deferred && c->deferred->active);
}
// (error paths and re-initialisation: the chunk's contents are unspecified while pieces are pending, so dropping them loses nothing)
static void drop_pending(qsim_chunk* c) {
  if (c->pending) c->pending->mode = PendingLast::kNone;
  if (c->deferred) c->deferred->active = false;
}
static int require_no_parts(const qsim_chunk* c, const char* what) {
  if (parts_pending(c)) return fail(QSIM_ERR_INVALID, "%s: slab pieces of a split qsim_apply_ops_io call are pending on this chunk", what);
  return QSIM_OK;
}
// An error between arming and disarming leaves nothing pending on the chunk.
struct PendingGuard {
  qsim_chunk* c;
  bool armed;
  ~PendingGuard() { if (armed) drop_pending(c); }
};
