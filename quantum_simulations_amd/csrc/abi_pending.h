// abi_pending.h -- what calls leave pending on a chunk.  A split qsim_apply_ops_io call (abi_relayout.h): the piece cut and the
// one record behind qsim_chunk::split; every topic of the C ABI asks whether pieces are pending.  A cyclic plan
// (abi_gates.h qsim_apply_cycle): the deferred tail behind qsim_chunk::deferred, and settle(), which runs it.
// Part of the single translation unit qsim_hip.hip (included there, in order; not a standalone header).

// The top nb index bits of a k-bit index that are none of the m slab bits, ascending (the piece bits of the split form).
static void top_free_bits(int k, int m, const int32_t* slab_bits, int nb, int* out) {
  for (int b = k - 1, found = 0; b >= 0 && found < nb; --b) {
    bool slab = false;
    for (int i = 0; i < m; ++i) slab = slab || slab_bits[i] == b;
    if (!slab) out[nb - 1 - found++] = b;
  }
}

// The slabs of a split call travel PIECE by piece: piece j = the j-th of 2^nb equal contiguous sub-ranges of EVERY slab
// (the top nb index bits that are not slab bits have the value j), so the exchange of piece j uses all links at once
// while the pieces behind it are still being computed.  The cut depends ONLY on (k, m, pieces asked for): every rank of a
// multi-GPU run cuts alike whatever its own pass plan looks like (ranks plan different op lists: rank-bit phases,
// controlled gates with a global control) -- the k-th transfer between two ranks always has the same size on both sides.
// What a rank's plan decides is only how early its pieces are ready: the top `nb_free` <= nb piece bits are no tile bits
// of the pass that stores (reads) the slabs, which then runs as 2^nb_free partial launches (a launch covers
// 2^(nb - nb_free) pieces; nb_free = 0: one launch).
struct PieceCut {
  int nb = 0;                        // piece bits: 2^nb pieces
  int piece_bit[3] = {0, 0, 0};      // the top nb non-slab index bits, ascending (piece j: bit i of j <-> piece_bit[i])
  int nb_free = 0;                   // how many of them, from the top, are no tile bits of the pass
  unsigned launched = 0;             // bit g: partial launch g (the top nb_free bits of the piece number) is queued

  // `parts` = 1, 2, 4, 8 asked for: as many as that while a piece keeps >= 2^20 amplitudes (negative: no such floor -- tests
  // cut small shards too) and whole 128-byte lines.  (`slab_bits` null: the count alone.)
  static PieceCut cut(int k, int m, const int32_t* slab_bits, int parts) {
    const int want = parts < 0 ? -parts : parts, min_piece_bits = parts < 0 ? kTileLow : 20;
    PieceCut c;
    while (c.nb < 3 && (2 << c.nb) <= want && (k - m) - (c.nb + 1) >= min_piece_bits && (k - m) - (c.nb + 1) >= kTileLow) ++c.nb;
    if (slab_bits) top_free_bits(k, m, slab_bits, c.nb, c.piece_bit);
    return c;
  }
  // the pass has the n high tile bits `tile_high`: the piece bits above all of them are free
  void free_above(const uint8_t* tile_high, int n) {
    auto is_tile = [&](int b) { for (int j = 0; j < n; ++j) if (tile_high[j] == b) return true; return false; };
    nb_free = 0;
    while (nb_free < nb && !is_tile(piece_bit[nb - 1 - nb_free])) ++nb_free;
  }
  int n_parts() const { return 1 << nb; }
  u64 piece_amps(int k, int m) const { return (1ull << (k - m)) >> nb; }
  int group_of(int part) const { return part >> (nb - nb_free); }      // the partial launch that covers piece `part`
};

// The record of a split call.  IN side (qsim_ops_io::src_parts, the receive side of a fused re-layout): the op list is
// planned and prepared at the call and launched as the source pieces are announced (qsim_apply_ops_io_load) -- the first
// pass as partial launches over the tiles whose source pieces are there, the rest when the source is complete.  OUT side
// (qsim_ops_io::dst_parts): the slabs are stored piece by piece (qsim_apply_ops_io_part) -- kTile: partial launches of the
// slab-storing pass, kept here instead of launched; kPack (nothing fusable: the state is final in the chunk): one
// qsim_pack_all piece per call; kDone: stored already (passes that cannot be launched in part).  A call with both has the
// in side live first; its last piece sets up the out side.
struct SplitIo {
  struct In {
    bool active = false;
    PieceCut cut;
    unsigned announced = 0;           // bit j: piece j has been handed in
    bool tiles = false;               // tile passes (else: chunk too small / no ops: gate by gate after the source is complete)
    std::vector<CachedPass> passes;   // prepared passes (buffers in)
    std::vector<int32_t> nq, qubits;  // the op list (kept for the gate-by-gate case)
    std::vector<double> mats;
    qsim_ops_io io;
    FusedIo fio;
  } in;
  struct Out {
    enum Mode { kNone = 0, kTile, kPack, kDone };
    int mode = kNone;
    PieceCut cut;
    unsigned stored = 0;              // bit j: piece j has been handed out
    CachedPass pass;                  // kTile: the slab-storing pass
    int m = 0;
    int32_t bits[3] = {0, 0, 0};
    qsim_chunk* dst = nullptr;
    qsim_chunk* dst_own = nullptr;
    int own_pattern = -1;
  } out;
};

static SplitIo* split_record(qsim_chunk* c) { return c->split ? c->split : (c->split = new SplitIo()); }
static bool parts_pending(const qsim_chunk* c) {
  return c->split && (c->split->in.active || c->split->out.mode != SplitIo::Out::kNone);
}
// (error paths and re-initialisation: the chunk's contents are unspecified while pieces are pending, so dropping them loses nothing)
static void drop_pending(qsim_chunk* c) {
  if (c->split) { c->split->in.active = false; c->split->out.mode = SplitIo::Out::kNone; }
}
static int require_no_parts(const qsim_chunk* c, const char* what) {
  if (parts_pending(c)) return fail(QSIM_ERR_INVALID, "%s: slab pieces of a split qsim_apply_ops_io call are pending on this chunk", what);
  return QSIM_OK;
}
// ---- the deferred tail of a cyclic plan (abi_gates.h qsim_apply_cycle) -------------------------------------------------------
// One execution of a cyclic plan leaves the passes of its tail B unlaunched on the chunk, so that the next execution can run
// them together with its head (B.A, a pass fewer than A and B apart).  The record shares the prepared passes with the cycle
// object (which may be destroyed first) and names it by `id`, never by address.  settle() launches what is deferred and
// clears the record: check_chunk calls it for every exported call (qsim_core.h), for a view also on the chunks it is a
// window of.  Only chunks that own their memory carry a tail, so no two chunks with one hide the same amplitudes.
typedef std::shared_ptr<const std::vector<CachedPass>> PassList;
struct DeferredTail {
  u64 id = 0;                        // the cycle whose tail it is
  PassList passes;                   // null: nothing deferred
};
static int launch_passes(qsim_chunk* c, const std::vector<CachedPass>& passes) {
  HIP_TRY(hipSetDevice(c->device));
  for (size_t p = 0; p < passes.size(); ++p) {
    CachedPass pass = passes[p];     // (buffers and launch geometry go into a copy: the images are shared)
    prepare_planned(c, pass.a, pass.T, p == 0, p + 1 == passes.size(), nullptr);
    const int rc = dispatch_planned(c, pass.a, pass.T, pass.alg_bytes);
    if (rc) return rc;
  }
  return QSIM_OK;
}
static void drop_deferred(qsim_chunk* c) {
  if (c->deferred) c->deferred->passes.reset();
}
static int settle(qsim_chunk* c) {
  for (; c; c = c->parent) {
    if (!c->deferred || !c->deferred->passes) continue;
    const PassList tail = std::move(c->deferred->passes);
    c->deferred->passes.reset();
    const int rc = launch_passes(c, *tail);
    if (rc) return rc;
  }
  return QSIM_OK;
}
// check_chunk of a call that overwrites every amplitude of the chunk: its own tail is dropped, not run
static int check_chunk_overwritten(qsim_chunk* c, const char* what) {
  const int rc = check_chunk_unsettled(c, what);
  if (rc) return rc;
  drop_deferred(c);
  return settle(c->parent);
}

// An error between arming and disarming leaves nothing pending on the chunk.
struct PendingGuard {
  qsim_chunk* c;
  bool armed;
  ~PendingGuard() { if (armed) drop_pending(c); }
};
