// abi_comm.h -- C ABI: the multi-GPU reach (comm_rccl.h): the communicator, exchanges in the foreground and in the
// background, the all-to-all re-layout (plain, loopback, fused into two op lists) and the remote butterflies.
// Part of the single translation unit qsim_hip.hip (included there, in order; not a standalone header).

static int check_exchange(const qsim_comm* cm, const char* what, int n_peers, const int32_t* peers, const qsim_chunk* send,
                          const uint64_t* send_off, const qsim_chunk* recv, const uint64_t* recv_off, uint64_t count_amps) {
  int rc = check_comm(cm, what);
  if (rc || (rc = check_chunk(send, what)) || (rc = check_chunk(recv, what))) return rc;
  if (n_peers < 0 || (n_peers && (!peers || !send_off || !recv_off))) return fail(QSIM_ERR_INVALID, "%s: bad peer list", what);
  if (send->amp == recv->amp) return fail(QSIM_ERR_INVALID, "%s: send and receive chunks must differ", what);
  if (send->stream != recv->stream) return fail(QSIM_ERR_INVALID, "%s: the send and the receive chunk must share a stream (the transfer is ordered on it)", what);
  for (int i = 0; i < n_peers; ++i) {
    if (peers[i] < 0 || peers[i] >= cm->world) return fail(QSIM_ERR_INVALID, "%s: peer %d out of range", what, peers[i]);
    if (send_off[i] > amps(send) || count_amps > amps(send) - send_off[i] || recv_off[i] > amps(recv) || count_amps > amps(recv) - recv_off[i])
      return fail(QSIM_ERR_INVALID, "%s: slice %d outside its chunk", what, i);
  }
  return QSIM_OK;
}

// The transfer stream and the events, made when first needed (with_bg_events: the tickets of qsim_comm_exchange_bg too).
static int ensure_xfer(qsim_comm* cm, bool with_bg_events) {
  if (!cm->xfer_stream) HIP_TRY(hipStreamCreateWithFlags(&cm->xfer_stream, hipStreamNonBlocking));
  for (auto& e : cm->ev) if (!e) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  if (with_bg_events)
    for (auto& e : cm->ev_bg) if (!e) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  return QSIM_OK;
}

extern "C" {
// ---- multi-GPU reach of the C ABI (comm_rccl.h) ---------------------------------------------------
int qsim_comm_get_unique_id(uint8_t id[QSIM_COMM_ID_BYTES]) {
  static_assert(QSIM_COMM_ID_BYTES == NCCL_UNIQUE_ID_BYTES, "unique id size");
  if (!id) return fail(QSIM_ERR_INVALID, "id is null");
  int rc = rccl_load();
  if (rc) return rc;
  ncclUniqueId uid;
  RCCL_TRY(g_rccl.GetUniqueId(&uid));
  std::memcpy(id, uid.internal, NCCL_UNIQUE_ID_BYTES);
  return QSIM_OK;
}

int qsim_comm_init(int device, int rank, int world, const uint8_t id[QSIM_COMM_ID_BYTES], qsim_comm** out) {
  if (!out || !id) return fail(QSIM_ERR_INVALID, "null argument");
  if (world < 1 || (world & (world - 1)) || rank < 0 || rank >= world)
    return fail(QSIM_ERR_INVALID, "qsim_comm_init: world %d must be a power of two and 0 <= rank %d < world", world, rank);
  int rc = rccl_load();
  if (rc) return rc;
  HIP_TRY(hipSetDevice(device));
  ncclUniqueId uid;
  std::memcpy(uid.internal, id, NCCL_UNIQUE_ID_BYTES);
  ncclComm_t comm = nullptr;
  RCCL_TRY(g_rccl.CommInitRank(&comm, world, uid, rank));
  qsim_comm* c = new qsim_comm();
  c->comm = comm; c->rank = rank; c->world = world; c->device = device;
  c->xfer_stream = nullptr;
  for (auto& e : c->ev) e = nullptr;
  for (auto& e : c->ev_bg) e = nullptr;
  c->bg_posted = 0;
  *out = c;
  return QSIM_OK;
}

int qsim_comm_destroy(qsim_comm* c) {
  if (!c) return QSIM_OK;
  (void)hipSetDevice(c->device);
  if (c->xfer_stream) { (void)hipStreamSynchronize(c->xfer_stream); (void)hipStreamDestroy(c->xfer_stream); }
  for (auto& e : c->ev) if (e) (void)hipEventDestroy(e);
  for (auto& e : c->ev_bg) if (e) (void)hipEventDestroy(e);
  if (c->comm && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(c->comm);
  delete c;
  return QSIM_OK;
}

int qsim_comm_rank(const qsim_comm* c) { return c ? c->rank : -1; }
int qsim_comm_world(const qsim_comm* c) { return c ? c->world : -1; }

int qsim_comm_exchange(qsim_comm* cm, int n_peers, const int32_t* peers, const qsim_chunk* send, const uint64_t* send_off,
                       qsim_chunk* recv, const uint64_t* recv_off, uint64_t count_amps) {
  int rc = check_exchange(cm, "qsim_comm_exchange", n_peers, peers, send, send_off, recv, recv_off, count_amps);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(cm->device));
  return comm_exchange(cm, n_peers, peers, send->amp, send_off, recv->amp, recv_off, count_amps, send->stream);
}

// Background form: the group is queued on the communicator's transfer stream behind everything queued on the chunks'
// stream SO FAR; what is queued on the chunks' stream later runs beside it.  qsim_comm_join makes a chunk's stream wait
// for every background transfer posted so far (the piece pipeline of a fused re-layout: runner/distributed.py).
int qsim_comm_exchange_bg(qsim_comm* cm, int n_peers, const int32_t* peers, const qsim_chunk* send, const uint64_t* send_off,
                          qsim_chunk* recv, const uint64_t* recv_off, uint64_t count_amps, uint32_t* ticket) {
  int rc = check_exchange(cm, "qsim_comm_exchange_bg", n_peers, peers, send, send_off, recv, recv_off, count_amps);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(cm->device));
  if ((rc = ensure_xfer(cm, true))) return rc;
  HIP_TRY(hipEventRecord(cm->ev[14], send->stream));
  HIP_TRY(hipStreamWaitEvent(cm->xfer_stream, cm->ev[14], 0));
  if ((rc = comm_exchange(cm, n_peers, peers, send->amp, send_off, recv->amp, recv_off, count_amps, cm->xfer_stream))) return rc;
  const uint32_t t = cm->bg_posted++;
  HIP_TRY(hipEventRecord(cm->ev_bg[t % 16], cm->xfer_stream));
  if (ticket) *ticket = t;
  return QSIM_OK;
}

// The chunk's stream waits for background exchange `ticket` (and, transfers of one communicator running in order, for
// every one posted before it) -- not for later ones: the pieces of a re-layout are consumed as they arrive.
int qsim_comm_wait(qsim_comm* cm, qsim_chunk* c, uint32_t ticket) {
  int rc = check_comm(cm, "qsim_comm_wait");
  if (rc || (rc = check_chunk(c, "qsim_comm_wait"))) return rc;
  if (ticket >= cm->bg_posted) return fail(QSIM_ERR_INVALID, "qsim_comm_wait: ticket %u has not been handed out", ticket);
  if (cm->bg_posted - ticket > 16) return qsim_comm_join(cm, c);   // its event has been reused: wait for everything posted
  HIP_TRY(hipSetDevice(cm->device));
  HIP_TRY(hipStreamWaitEvent(c->stream, cm->ev_bg[ticket % 16], 0));
  return QSIM_OK;
}

int qsim_comm_join(qsim_comm* cm, qsim_chunk* c) {
  int rc = check_comm(cm, "qsim_comm_join");
  if (rc || (rc = check_chunk(c, "qsim_comm_join"))) return rc;
  if (!cm->xfer_stream) return QSIM_OK;                     // nothing was ever posted in the background
  HIP_TRY(hipSetDevice(cm->device));
  HIP_TRY(hipEventRecord(cm->ev[15], cm->xfer_stream));
  HIP_TRY(hipStreamWaitEvent(c->stream, cm->ev[15], 0));
  return QSIM_OK;
}

// ---- all-to-all re-layout: ONE schedule, computed by a pure function --------------------------------------------
// Who sends what to whom when rank `rank` of `world` swaps its local bits local_bits[i] with the rank bits
// global_bits[i] (bit g of the rank = qubit k + g): the partner semantics of the reference's chunk groups
// (wenbo_engine/runner/single_node.py:222-245) with one chunk per rank.  Slab d of the send buffer (offset d * 2^(k-m):
// this rank's amplitudes whose local bits have the pattern d) goes to the rank whose global-bit pattern is d, and that
// rank's slab `own` (own = this rank's pattern) arrives at the same offset d of the receive buffer; the own slab stays.
// Pieces: every slab is cut into n_pieces equal parts that travel one after the other (pack / transfer / unpack overlap).
struct RelayoutPlan {
  int n_pieces, n_peers, own;
  int32_t peers[7];
  uint64_t offs[7];          // amplitude offset of the peer's slab in the send AND the receive buffer
  uint64_t slab, part;       // amplitudes per slab / per piece
};
static int relayout_plan(int rank, int world, int k, int m, const int32_t* local_bits, const int32_t* global_bits, int n_pieces, RelayoutPlan* p) {
  if (world < 1 || (world & (world - 1)) || rank < 0 || rank >= world) return fail(QSIM_ERR_INVALID, "re-layout: bad rank %d / world %d", rank, world);
  if (m < 1 || m > 3 || !local_bits || !global_bits) return fail(QSIM_ERR_INVALID, "re-layout: 1..3 qubit pairs expected, got %d", m);
  int g_bits = 0;
  while ((1 << g_bits) < world) ++g_bits;
  const int rc = check_swapped_bits(k, g_bits, m, local_bits, global_bits, "re-layout", "shards", "rank bit");
  if (rc) return rc;
  if (n_pieces != 1 && n_pieces != 2 && n_pieces != 4 && n_pieces != 8) return fail(QSIM_ERR_INVALID, "re-layout: n_pieces must be 1, 2, 4 or 8");
  n_pieces = PieceCut::cut(k, m, local_bits, n_pieces).n_parts();      // pieces stay >= 2^20 amplitudes: the rule of the split form
  p->n_pieces = n_pieces;
  p->own = 0;
  for (int i = 0; i < m; ++i) p->own |= ((rank >> global_bits[i]) & 1) << i;
  p->slab = 1ull << (k - m);
  p->part = p->slab / (u64)n_pieces;
  p->n_peers = 0;
  for (int d = 0; d < (1 << m); ++d) {
    if (d == p->own) continue;
    p->peers[p->n_peers] = peer_of(rank, m, global_bits, d);
    p->offs[p->n_peers] = (u64)d * p->slab;
    ++p->n_peers;
  }
  return QSIM_OK;
}

int qsim_comm_relayout_plan(int rank, int world, int n_local_qubits, int m, const int32_t* local_bits, const int32_t* global_bits,
                            int n_pieces, int32_t* out_n_pieces, int32_t* out_n_peers, int32_t* out_own_pattern,
                            int32_t* out_peers, uint64_t* out_slab_offsets, uint64_t* out_piece_amps) {
  RelayoutPlan p;
  int rc = relayout_plan(rank, world, n_local_qubits, m, local_bits, global_bits, n_pieces, &p);
  if (rc) return rc;
  if (out_n_pieces) *out_n_pieces = p.n_pieces;
  if (out_n_peers) *out_n_peers = p.n_peers;
  if (out_own_pattern) *out_own_pattern = p.own;
  for (int i = 0; i < p.n_peers; ++i) {
    if (out_peers) out_peers[i] = p.peers[i];
    if (out_slab_offsets) out_slab_offsets[i] = p.offs[i];
  }
  if (out_piece_amps) *out_piece_amps = p.part;
  return QSIM_OK;
}

// pipeline: pack piece s+1 (chunk stream) while piece s is on the links (transfer stream); unpack behind it.
// loopback: every peer is this rank itself (the slabs come back unchanged): the same packs, events, streams, RCCL
// groups and unpacks as a real re-layout of the planned rank, runnable on one GPU.
static int relayout_run(qsim_comm* cm, qsim_chunk* state, qsim_chunk* buf0, qsim_chunk* buf1, int m, const int32_t* local_bits,
                        const RelayoutPlan& p, bool loopback) {
  int rc = QSIM_OK;
  if (buf0->k != state->k || buf1->k != state->k || buf0->amp == buf1->amp || buf0->amp == state->amp || buf1->amp == state->amp)
    return fail(QSIM_ERR_INVALID, "re-layout: two distinct exchange buffers of the shard's size are needed");
  HIP_TRY(hipSetDevice(cm->device));
  if ((rc = ensure_xfer(cm, false))) return rc;
  int32_t peers[7];
  for (int i = 0; i < p.n_peers; ++i) peers[i] = loopback ? cm->rank : p.peers[i];
  for (int s = 0; s < p.n_pieces; ++s) {
    if ((rc = slabs_all(state, m, local_bits, buf0, p.own, s, p.n_pieces, true, "qsim_comm_relayout"))) return rc;
    HIP_TRY(hipEventRecord(cm->ev[2 * s], state->stream));
    HIP_TRY(hipStreamWaitEvent(cm->xfer_stream, cm->ev[2 * s], 0));
    uint64_t so[7];
    for (int i = 0; i < p.n_peers; ++i) so[i] = p.offs[i] + (u64)s * p.part;
    if ((rc = comm_exchange(cm, p.n_peers, peers, buf0->amp, so, buf1->amp, so, p.part, cm->xfer_stream))) return rc;
    HIP_TRY(hipEventRecord(cm->ev[2 * s + 1], cm->xfer_stream));
  }
  for (int s = 0; s < p.n_pieces; ++s) {
    HIP_TRY(hipStreamWaitEvent(state->stream, cm->ev[2 * s + 1], 0));
    if ((rc = slabs_all(state, m, local_bits, buf1, p.own, s, p.n_pieces, false, "qsim_comm_relayout"))) return rc;
  }
  return QSIM_OK;
}

static int relayout_as(qsim_comm* cm, qsim_chunk* state, qsim_chunk* buf0, qsim_chunk* buf1, int m, const int32_t* local_bits,
                       const int32_t* global_bits, int n_pieces, int rank, int world, bool loopback, const char* what) {
  int rc = check_comm(cm, what);
  if (rc || (rc = check_chunk(state, what)) || (rc = check_chunk(buf0, what)) || (rc = check_chunk(buf1, what))) return rc;
  RelayoutPlan p;
  if ((rc = relayout_plan(rank, world, state->k, m, local_bits, global_bits, n_pieces, &p))) return rc;
  return relayout_run(cm, state, buf0, buf1, m, local_bits, p, loopback);
}

// All-to-all re-layout of THIS rank's shard: local bits `local_bits[i]` trade places with rank bits
// `global_bits[i]` (bit g of the rank = qubit k + g).  buf0 / buf1: exchange buffers of the shard's size.
int qsim_comm_relayout(qsim_comm* cm, qsim_chunk* state, qsim_chunk* buf0, qsim_chunk* buf1, int m,
                       const int32_t* local_bits, const int32_t* global_bits, int n_pieces) {
  int rc = check_comm(cm, "qsim_comm_relayout");
  if (rc) return rc;
  return relayout_as(cm, state, buf0, buf1, m, local_bits, global_bits, n_pieces, cm->rank, cm->world, false, "qsim_comm_relayout");
}

// The pipeline of qsim_comm_relayout as rank `as_rank` of a world of `as_world` would run it, with every transfer
// looped back to this rank: the state is unchanged afterwards and buf1 holds the slabs that were "received".
int qsim_comm_relayout_loopback(qsim_comm* cm, qsim_chunk* state, qsim_chunk* buf0, qsim_chunk* buf1, int m,
                                const int32_t* local_bits, const int32_t* global_bits, int n_pieces, int as_rank, int as_world) {
  return relayout_as(cm, state, buf0, buf1, m, local_bits, global_bits, n_pieces, as_rank, as_world, true, "qsim_comm_relayout_loopback");
}

// The fused re-layout as ONE call for a host without the Python runner (what runner/distributed.py does with
// qsim_apply_ops_io + its own exchange): shard := after( re-layout( before(shard) ) ).  The last fused pass of `before`
// stores the slabs piece by piece (qsim_ops_io::dst_parts) on the chunk's stream; the exchange of piece j -- every peer in
// one RCCL group, all links busy -- runs on the communicator's transfer stream as soon as piece j is stored, while piece
// j + 1 is computed; the first pass of `after` reads the received slabs from `recv`.  Two HBM passes fewer than
// qsim_comm_relayout between two op lists, and the compute of all pieces but the first hidden behind the links.
int qsim_comm_relayout_fused(qsim_comm* cm, qsim_chunk* shard, qsim_chunk* send, qsim_chunk* recv,
                             const qsim_op_list* before, const qsim_op_list* after, int m, const int32_t* local_bits,
                             const int32_t* global_bits, int n_pieces, int as_rank, int as_world, int* n_passes) {
  int rc = check_comm(cm, "qsim_comm_relayout_fused");
  if (rc || (rc = check_chunk(shard, "qsim_comm_relayout_fused")) || (rc = check_chunk(send, "qsim_comm_relayout_fused")) ||
      (rc = check_chunk(recv, "qsim_comm_relayout_fused"))) return rc;
  if (send->stream != shard->stream || recv->stream != shard->stream)
    return fail(QSIM_ERR_INVALID, "qsim_comm_relayout_fused: the shard and both buffers must share a stream");
  const bool loopback = as_world != 0;
  RelayoutPlan p;
  if ((rc = relayout_plan(loopback ? as_rank : cm->rank, loopback ? as_world : cm->world, shard->k, m, local_bits, global_bits, 1, &p))) return rc;
  static const qsim_op_list none = {0, nullptr, nullptr, nullptr};
  if (!before) before = &none;
  if (!after) after = &none;
  if (n_pieces != 1 && n_pieces != 2 && n_pieces != 4 && n_pieces != 8 && n_pieces != -2 && n_pieces != -4 && n_pieces != -8)
    return fail(QSIM_ERR_INVALID, "qsim_comm_relayout_fused: n_pieces must be 1, 2, 4 or 8");
  HIP_TRY(hipSetDevice(cm->device));
  if ((rc = ensure_xfer(cm, false))) return rc;
  qsim_ops_io io;
  std::memset(&io, 0, sizeof io);
  io.struct_size = sizeof io;
  io.dst = send; io.dst_m = m; io.dst_own = recv; io.own_pattern = p.own;
  for (int i = 0; i < m; ++i) io.dst_bits[i] = local_bits[i];
  io.dst_parts = n_pieces == 1 ? -1 : n_pieces;            // (always the split form: -1 = one piece)
  int passes_before = 0, passes_after = 0;
  if ((rc = qsim_apply_ops_io(shard, before->n_ops, before->nq, before->qubits, before->mats, &io, &passes_before))) return rc;
  int32_t n_parts = 0;
  uint64_t piece_amps = 0;
  PendingGuard guard{shard, true};     // an error below leaves nothing pending
  if ((rc = qsim_apply_ops_io_parts(shard, &n_parts, &piece_amps, nullptr))) return rc;
  for (int j = 0; j < n_parts; ++j) {
    if ((rc = qsim_apply_ops_io_part(shard, j))) return rc;
    HIP_TRY(hipEventRecord(cm->ev[j], shard->stream));
    HIP_TRY(hipStreamWaitEvent(cm->xfer_stream, cm->ev[j], 0));
    int32_t peers[8];
    uint64_t offs[8];
    for (int i = 0; i < p.n_peers; ++i) {
      peers[i] = loopback ? cm->rank : p.peers[i];
      offs[i] = p.offs[i] + (u64)j * piece_amps;
    }
    if ((rc = comm_exchange(cm, p.n_peers, peers, send->amp, offs, recv->amp, offs, piece_amps, cm->xfer_stream))) return rc;
    HIP_TRY(hipEventRecord(cm->ev[8 + j], cm->xfer_stream));       // piece j has arrived
  }
  // receive side: `after` is planned now (the links are busy meanwhile) and takes the pieces over as they arrive -- its
  // first pass runs on the tiles whose pieces are there, the rest with the last piece
  std::memset(&io, 0, sizeof io);
  io.struct_size = sizeof io;
  io.src = recv; io.src_m = m; io.own_pattern = -1;
  for (int i = 0; i < m; ++i) io.src_bits[i] = local_bits[i];
  io.src_parts = n_pieces == 1 ? -1 : n_pieces;
  if ((rc = qsim_apply_ops_io(shard, after->n_ops, after->nq, after->qubits, after->mats, &io, &passes_after))) return rc;
  int32_t n_in = 0;
  if ((rc = qsim_apply_ops_io_source_parts(shard, &n_in, nullptr, nullptr))) return rc;
  if (n_in != n_parts) return fail(QSIM_ERR_INVALID, "internal: %d source pieces for %d sent ones", n_in, n_parts);
  for (int j = 0; j < n_parts; ++j) {
    HIP_TRY(hipStreamWaitEvent(shard->stream, cm->ev[8 + j], 0));
    if ((rc = qsim_apply_ops_io_load(shard, j))) return rc;
  }
  guard.armed = false;
  if (n_passes) *n_passes = passes_before + passes_after;
  return QSIM_OK;
}

// cpu_nonlocal.apply_2q_quad (cpu_nonlocal.py:61-67; chunk groups of four, single_node.py:315-321) with the four chunks
// on four ranks: ranks[j] holds chunk j = 2 bit(qa) + bit(qb) (the argument order c00, c01, c10, c11) and this rank is
// ranks[my_index].  The local index range is cut into four quarters and every taking-part rank WORKS ON some of them: it
// receives those quarters of its partners' shards into `buf`, applies the matrix across the copies and its own quarter,
// and sends the results back -- 3/4 of a shard each way, twice, instead of three whole shards in.  A chunk the matrix
// leaves alone (its row and column are the identity's: the |0x> chunks of a gate controlled by qa) takes no part: its
// rank returns at once, nobody sends to it or waits for it (two active chunks: a 2x2 across the pair, half a shard each
// way).  ranks = {r, r, r, r} with r = this rank is the one-GPU loopback form: every transfer comes back, so the gate
// acts on the shard's own four quarters (chunk j = quarter j: local qubits k - 1 and k - 2).
int qsim_apply_2q_quad_remote(qsim_comm* cm, qsim_chunk* shard, qsim_chunk* buf, const int32_t ranks[4], int my_index, const double U[32]) {
  const char* what = "qsim_apply_2q_quad_remote";
  int rc = check_comm(cm, what);
  if (rc || (rc = check_chunk(shard, what)) || (rc = check_chunk(buf, what))) return rc;
  if (!ranks || !U) return fail(QSIM_ERR_INVALID, "%s: null argument", what);
  if (buf->k != shard->k || buf->amp == shard->amp || buf->stream != shard->stream)
    return fail(QSIM_ERR_INVALID, "%s: the buffer must be a distinct chunk of the shard's size on the shard's stream", what);
  if (shard->k < 2) return fail(QSIM_ERR_INVALID, "%s: shards of at least 4 amplitudes are needed", what);
  if (my_index < 0 || my_index > 3) return fail(QSIM_ERR_INVALID, "%s: my_index must be 0..3", what);
  bool loopback = true;
  for (int j = 0; j < 4; ++j) {
    if (ranks[j] < 0 || ranks[j] >= cm->world) return fail(QSIM_ERR_INVALID, "%s: rank %d out of range", what, ranks[j]);
    loopback = loopback && ranks[j] == cm->rank;
  }
  if (!loopback) {
    if (ranks[my_index] != cm->rank) return fail(QSIM_ERR_INVALID, "%s: ranks[my_index] must be this rank", what);
    for (int j = 0; j < 4; ++j)
      for (int i = 0; i < j; ++i)
        if (ranks[i] == ranks[j]) return fail(QSIM_ERR_INVALID, "%s: the four chunks live on four different ranks (or all on this one: loopback)", what);
  }
  // chunks the matrix touches (a unitary touches none, or at least two; exactly three: treated as all four)
  int act[4], n_act = 0;
  bool active[4];
  for (int j = 0; j < 4; ++j) {
    bool unit = true;
    for (int c = 0; c < 4; ++c) {
      const double want = c == j ? 1.0 : 0.0;
      unit = unit && U[2 * (4 * j + c)] == want && U[2 * (4 * j + c) + 1] == 0.0 && U[2 * (4 * c + j)] == want && U[2 * (4 * c + j) + 1] == 0.0;
    }
    active[j] = !unit;
  }
  for (int j = 0; j < 4; ++j) n_act += active[j];
  if (n_act == 0) return QSIM_OK;
  if (n_act == 3) { n_act = 4; for (bool& a : active) a = true; }
  if (!active[my_index]) return QSIM_OK;
  if (n_act == 1) {                                        // a phase on one chunk (CZ, CR with both qubits global): no exchange
    const double f[8] = {U[2 * (5 * my_index)], U[2 * (5 * my_index) + 1], 0, 0, 0, 0, U[2 * (5 * my_index)], U[2 * (5 * my_index) + 1]};
    return qsim_apply_1q(shard, 0, f);
  }
  for (int j = 0, i = 0; j < 4; ++j) if (active[j]) act[i++] = j;
  HIP_TRY(hipSetDevice(cm->device));
  const u64 Q = amps(shard) >> 2;
  auto owner = [&](int q) { return act[q % n_act]; };      // the chunk whose rank works on quarter q
  auto slot_of = [&](int q, int j) -> u64 {                 // where partner chunk j's quarter q sits in MY buffer (I work on q)
    u64 s = 0;
    for (int qq = 0; qq < 4; ++qq) {
      if (owner(qq) != my_index) continue;
      for (int i = 0; i < n_act; ++i) {
        if (act[i] == my_index) continue;
        if (qq == q && act[i] == j) return s;
        ++s;
      }
    }
    return 0;                                               // (unreachable)
  };
  // One RCCL group per direction.  Between two ranks the k-th send meets the k-th receive: both sides walk the quarters in
  // ascending order (and, inside a quarter, the partners in ascending chunk order).
  auto exchange = [&](bool back) -> int {
    RCCL_TRY(g_rccl.GroupStart());
    ncclResult_t bad = ncclSuccess;
    for (int q = 0; q < 4 && bad == ncclSuccess; ++q) {
      const int o = owner(q);
      if (o == my_index) {                                  // partners' copies of quarter q: in (there) / out (back)
        for (int i = 0; i < n_act && bad == ncclSuccess; ++i) {
          if (act[i] == my_index) continue;
          double2* copy = buf->amp + slot_of(q, act[i]) * Q;
          bad = back ? g_rccl.Send(copy, 2 * Q, ncclDouble, ranks[act[i]], cm->comm, shard->stream)
                     : g_rccl.Recv(copy, 2 * Q, ncclDouble, ranks[act[i]], cm->comm, shard->stream);
        }
      } else {                                              // my quarter q: out to the rank that works on it / back in
        double2* mine = shard->amp + (u64)q * Q;
        bad = back ? g_rccl.Recv(mine, 2 * Q, ncclDouble, ranks[o], cm->comm, shard->stream)
                   : g_rccl.Send(mine, 2 * Q, ncclDouble, ranks[o], cm->comm, shard->stream);
      }
    }
    const ncclResult_t end = g_rccl.GroupEnd();             // (closed on every path)
    if (bad != ncclSuccess) return fail(QSIM_ERR_HIP, "%s: RCCL send / receive failed: %s", what, g_rccl.GetErrorString(bad));
    if (end != ncclSuccess) return fail(QSIM_ERR_HIP, "%s: ncclGroupEnd failed: %s", what, g_rccl.GetErrorString(end));
    return QSIM_OK;
  };
  if ((rc = exchange(false))) return rc;
  for (int q = 0; q < 4; ++q) {
    if (owner(q) != my_index) continue;
    qsim_chunk view[4];
    for (int j = 0; j < 4; ++j) {
      view[j] = *shard;                                     // device, stream, cache policy of the shard's allocation
      view[j].k = shard->k - 2;
      view[j].owns_memory = false; view[j].scratch = nullptr; view[j].work = nullptr; view[j].work_bytes = 0; view[j].have_events = false; view[j].split = nullptr;
      view[j].amp = j == my_index ? shard->amp + (u64)q * Q : (active[j] ? buf->amp + slot_of(q, j) * Q : nullptr);
    }
    if (n_act == 4) {
      Group g = {{&view[0], &view[1], &view[2], &view[3]}, 4, shard->k - 2};
      if ((rc = gate_2q(g, shard->k - 1, shard->k - 2, U, shard->stream))) return rc;
    } else {                                                // two active chunks a < b: the 2x2 [[U_aa, U_ab], [U_ba, U_bb]] across the pair
      const int a = act[0], b = act[1];
      const double W[8] = {U[2 * (4 * a + a)], U[2 * (4 * a + a) + 1], U[2 * (4 * a + b)], U[2 * (4 * a + b) + 1],
                           U[2 * (4 * b + a)], U[2 * (4 * b + a) + 1], U[2 * (4 * b + b)], U[2 * (4 * b + b) + 1]};
      Group g = {{&view[a], &view[b], nullptr, nullptr}, 2, shard->k - 2};
      if ((rc = gate_1q(g, shard->k - 2, W, shard->stream))) return rc;
    }
  }
  return exchange(true);
}

// The reference's partner-chunk butterflies with the partner chunk on ANOTHER rank: both ranks call with each
// other's rank; `my_side` = this rank's value of the global qubit (0: this shard is c0, 1: it is c1).  The
// partner's whole shard is received into `buf` and the pair kernel updates this rank's shard (the copy in
// `buf` is scratch afterwards).
static int pair_remote(qsim_comm* cm, qsim_chunk* shard, qsim_chunk* buf, int partner, int my_side, const char* what) {
  int rc = check_comm(cm, what);
  if (rc || (rc = check_chunk(shard, what)) || (rc = check_chunk(buf, what))) return rc;
  if (buf->k != shard->k || buf->amp == shard->amp) return fail(QSIM_ERR_INVALID, "%s: the receive buffer must be a distinct chunk of the shard's size", what);
  if (partner < 0 || partner >= cm->world) return fail(QSIM_ERR_INVALID, "%s: partner rank %d out of range", what, partner);
  if (my_side != 0 && my_side != 1) return fail(QSIM_ERR_INVALID, "%s: my_side must be 0 or 1", what);
  HIP_TRY(hipSetDevice(cm->device));
  const int32_t peer = partner;
  const uint64_t zero = 0;
  return comm_exchange(cm, 1, &peer, shard->amp, &zero, buf->amp, &zero, amps(shard), shard->stream);
}

int qsim_apply_1q_pair_remote(qsim_comm* cm, qsim_chunk* shard, qsim_chunk* buf, int partner_rank, int my_side, const double U[8]) {
  int rc = pair_remote(cm, shard, buf, partner_rank, my_side, "qsim_apply_1q_pair_remote");
  if (rc) return rc;
  return my_side == 0 ? qsim_apply_1q_pair(shard, buf, U) : qsim_apply_1q_pair(buf, shard, U);
}

int qsim_apply_2q_pair_qa_local_remote(qsim_comm* cm, qsim_chunk* shard, qsim_chunk* buf, int partner_rank, int my_side, int qa, const double U[32]) {
  int rc = pair_remote(cm, shard, buf, partner_rank, my_side, "qsim_apply_2q_pair_qa_local_remote");
  if (rc) return rc;
  return my_side == 0 ? qsim_apply_2q_pair_qa_local(shard, buf, qa, U) : qsim_apply_2q_pair_qa_local(buf, shard, qa, U);
}

int qsim_apply_2q_pair_qb_local_remote(qsim_comm* cm, qsim_chunk* shard, qsim_chunk* buf, int partner_rank, int my_side, int qb, const double U[32]) {
  int rc = pair_remote(cm, shard, buf, partner_rank, my_side, "qsim_apply_2q_pair_qb_local_remote");
  if (rc) return rc;
  return my_side == 0 ? qsim_apply_2q_pair_qb_local(shard, buf, qb, U) : qsim_apply_2q_pair_qb_local(buf, shard, qb, U);
}
}  // extern "C"
