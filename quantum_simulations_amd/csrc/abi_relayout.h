// abi_relayout.h -- C ABI: slab packing (the two ends of an all-to-all re-layout), the in-place swap between chunks of one
// device, and qsim_apply_ops_io: an op list with the re-layout fused into its ends, whole or in pieces (_part / _load).
// Part of the single translation unit qsim_hip.hip (included there, in order; not a standalone header).
#include "slab_kernels.h"

// The m (local bit, rank bit) pairs of a re-layout: in range and distinct (`what`, `shards`, `index_bit`: the caller's words).
static int check_swapped_bits(int k, int g_bits, int m, const int32_t* local_bits, const int32_t* global_bits, const char* what,
                              const char* shards, const char* index_bit) {
  for (int i = 0; i < m; ++i) {
    if (local_bits[i] < 0 || local_bits[i] >= k) return fail(QSIM_ERR_NONLOCAL, "%s: local bit %d is non-local for 2^%d %s", what, local_bits[i], k, shards);
    if (global_bits[i] < 0 || global_bits[i] >= g_bits) return fail(QSIM_ERR_INVALID, "%s: %s %d out of range", what, index_bit, global_bits[i]);
    for (int j = 0; j < i; ++j)
      if (local_bits[j] == local_bits[i] || global_bits[j] == global_bits[i]) return fail(QSIM_ERR_INVALID, "%s: repeated bit", what);
  }
  return QSIM_OK;
}
// The first of m slab bits that lies outside [0, k) or (*repeated) repeats an earlier one, in list order; -1: none does.
static int bad_slab_bit(int k, int m, const int32_t* bits, bool* repeated) {
  for (int i = 0; i < m; ++i) {
    *repeated = false;
    if (bits[i] < 0 || bits[i] >= k) return i;
    *repeated = true;
    for (int j = 0; j < i; ++j) if (bits[j] == bits[i]) return i;
  }
  return -1;
}
// The rank (chunk index) that differs from `rank` in having pattern d on the swapped index bits.
static int peer_of(int rank, int m, const int32_t* global_bits, int d) {
  for (int i = 0; i < m; ++i) rank = (rank & ~(1 << global_bits[i])) | (((d >> i) & 1) << global_bits[i]);
  return rank;
}

// The launch of a planned pass on the tiles of ONE value g of its n_free top piece bits (piece_bits, ascending; no tile bits).
static int partial_launch_args(const TileArgs& planned, int T, int k, const int* piece_bits, int n_free, int g, TileArgs* out) {
  *out = planned;
  out->nfix = (uint8_t)n_free;
  out->fix_or = 0;
  for (int i = 0; i < n_free; ++i) {
    const int bit = piece_bits[i];
    int below = 0;
    for (int j = 0; j < T - kTileLow; ++j) below += out->h[j] < bit;
    out->fix_pos[i] = (uint8_t)(bit - below);
    if ((g >> i) & 1) out->fix_or |= 1ull << bit;
    if (bit >= k || bit < kTileLow) return fail(QSIM_ERR_INVALID, "internal: piece bit %d", bit);
  }
  return QSIM_OK;
}
// Partial launch g of a kept pass, unless it is queued already: the tiles whose top cut.nb_free piece bits have the value g.
static int launch_group(qsim_chunk* c, const CachedPass& p, PieceCut& cut, int g) {
  if ((cut.launched >> g) & 1) return QSIM_OK;
  TileArgs a;
  int rc = partial_launch_args(p.a, p.T, c->k, cut.piece_bit + (cut.nb - cut.nb_free), cut.nb_free, g, &a);
  if (rc || (rc = launch_tile_any(a, p.T, c, c->stream, p.alg_bytes / (double)(1 << cut.nb_free)))) return rc;
  cut.launched |= 1u << g;
  return QSIM_OK;
}

extern "C" {
// the half of `state` whose index bit `bit` has the given value <-> the half-sized chunk `buf`
static int half_slab(qsim_chunk* state, int bit, int value, qsim_chunk* buf, bool pack, const char* what) {
  int rc = check_chunk(state, what);
  if (rc || (rc = check_chunk(buf, what))) return rc;
  if (bit < 0 || bit >= state->k || buf->k != state->k - 1 || (value != 0 && value != 1))
    return fail(QSIM_ERR_INVALID, "%s: bit %d / buffer size mismatch", what, bit);
  HIP_TRY(hipSetDevice(state->device));
  const u64 n_half = amps(buf), off = value ? (1ull << bit) : 0ull;
  if (pack) hipLaunchKernelGGL(k_pack_half, dim3(stream_grid(n_half)), dim3(kBlock), 0, state->stream, buf->amp, (const double2*)state->amp, n_half, bit, off);
  else hipLaunchKernelGGL(k_unpack_half, dim3(stream_grid(n_half)), dim3(kBlock), 0, state->stream, state->amp, (const double2*)buf->amp, n_half, bit, off);
  HIP_TRY(hipGetLastError());
  return QSIM_OK;
}
int qsim_pack_half(const qsim_chunk* src, int bit, int value, qsim_chunk* buf) {
  return half_slab(const_cast<qsim_chunk*>(src), bit, value, buf, true, "qsim_pack_half");
}
int qsim_unpack_half(qsim_chunk* dst, int bit, int value, const qsim_chunk* buf) {
  return half_slab(dst, bit, value, const_cast<qsim_chunk*>(buf), false, "qsim_unpack_half");
}

static int slab_args(const qsim_chunk* c, int m, const int32_t* bits, int pattern, const qsim_chunk* buf,
                     uint64_t buf_offset, int pos[3], u64* value_off, u64* n_slab) {
  if (m < 1 || m > 3 || !bits) return fail(QSIM_ERR_INVALID, "slab: 1..3 bits expected, got %d", m);
  if (m > c->k) return fail(QSIM_ERR_INVALID, "slab: more bits than the chunk has");
  if (pattern < 0 || pattern >= (1 << m)) return fail(QSIM_ERR_INVALID, "slab: pattern out of range");
  int sorted[3] = {0, 0, 0};
  *value_off = 0;
  bool repeated;
  if (const int i = bad_slab_bit(c->k, m, bits, &repeated); i >= 0)
    return repeated ? fail(QSIM_ERR_INVALID, "slab: repeated bit %d", bits[i]) : fail(QSIM_ERR_INVALID, "slab: bit %d out of range", bits[i]);
  for (int i = 0; i < m; ++i) {
    sorted[i] = bits[i];
    if ((pattern >> i) & 1) *value_off |= 1ull << bits[i];
  }
  std::sort(sorted, sorted + m);
  for (int i = 0; i < 3; ++i) pos[i] = sorted[i];
  *n_slab = 1ull << (c->k - m);
  if (buf_offset > amps(buf) || *n_slab > amps(buf) - buf_offset)
    return fail(QSIM_ERR_INVALID, "slab: buffer range outside the buffer chunk");
  return QSIM_OK;
}

// slab `pattern` of `state` over `bits` <-> buf[buf_offset_amps, + 2^(k - m))
static int one_slab(qsim_chunk* state, int m, const int32_t* bits, int pattern, qsim_chunk* buf, uint64_t buf_offset_amps,
                    bool pack, const char* what) {
  int rc = check_chunk(state, what);
  if (rc || (rc = check_chunk(buf, what))) return rc;
  int pos[3];
  u64 voff, n_slab;
  if ((rc = slab_args(state, m, bits, pattern, buf, buf_offset_amps, pos, &voff, &n_slab))) return rc;
  HIP_TRY(hipSetDevice(state->device));
  if (pack) hipLaunchKernelGGL(k_pack_bits, dim3(stream_grid(n_slab)), dim3(kBlock), 0, state->stream,
                               buf->amp + buf_offset_amps, (const double2*)state->amp, n_slab, m, pos[0], pos[1], pos[2], voff);
  else hipLaunchKernelGGL(k_unpack_bits, dim3(stream_grid(n_slab)), dim3(kBlock), 0, state->stream,
                          state->amp, (const double2*)buf->amp + buf_offset_amps, n_slab, m, pos[0], pos[1], pos[2], voff);
  HIP_TRY(hipGetLastError());
  return QSIM_OK;
}
int qsim_pack_bits(const qsim_chunk* src, int m, const int32_t* bits, int pattern, qsim_chunk* buf, uint64_t buf_offset_amps) {
  return one_slab(const_cast<qsim_chunk*>(src), m, bits, pattern, buf, buf_offset_amps, true, "qsim_pack_bits");
}
int qsim_unpack_bits(qsim_chunk* dst, int m, const int32_t* bits, int pattern, const qsim_chunk* buf, uint64_t buf_offset_amps) {
  return one_slab(dst, m, bits, pattern, const_cast<qsim_chunk*>(buf), buf_offset_amps, false, "qsim_unpack_bits");
}

static int slabs_all(qsim_chunk* state, int m, const int32_t* bits, qsim_chunk* buf, int skip_pattern, int piece,
                     int n_pieces, bool pack, const char* what) {
  int rc = check_chunk(state, what);
  if (rc || (rc = check_chunk(buf, what))) return rc;
  int pos[3];
  u64 voff, n_slab;
  if ((rc = slab_args(state, m, bits, 0, buf, 0, pos, &voff, &n_slab))) return rc;
  if (amps(buf) < amps(state)) return fail(QSIM_ERR_INVALID, "%s: the buffer must hold all 2^%d slabs", what, m);
  if (skip_pattern < -1 || skip_pattern >= (1 << m)) return fail(QSIM_ERR_INVALID, "%s: skip pattern out of range", what);
  int piece_bits = 0;
  while ((1 << piece_bits) < n_pieces) ++piece_bits;
  if (n_pieces < 1 || (1 << piece_bits) != n_pieces || piece_bits > 3 || piece_bits > state->k - m)
    return fail(QSIM_ERR_INVALID, "%s: n_pieces must be 1, 2, 4 or 8 and at most the slab length", what);
  if (piece < 0 || piece >= n_pieces) return fail(QSIM_ERR_INVALID, "%s: piece %d out of range", what, piece);
  int pb[3] = {0, 0, 0};
  top_free_bits(state->k, m, bits, piece_bits, pb);
  HIP_TRY(hipSetDevice(state->device));
  const int b0 = bits[0], b1 = m > 1 ? bits[1] : 0, b2 = m > 2 ? bits[2] : 0;
  const int s_lo = pos[0], s_mid = m > 1 ? pos[1] : 0, s_hi = m > 2 ? pos[2] : 0;   // pos is sorted ascending
  const u64 n = amps(state) >> piece_bits;
  if (pack)
    hipLaunchKernelGGL((k_slabs_all<true>), dim3(stream_grid(n)), dim3(kBlock), 0, state->stream, state->amp, buf->amp,
                       n, m, b0, b1, b2, s_hi, s_mid, s_lo, state->k - m, skip_pattern, piece_bits, pb[0], pb[1], pb[2], piece);
  else
    hipLaunchKernelGGL((k_slabs_all<false>), dim3(stream_grid(n)), dim3(kBlock), 0, state->stream, state->amp, buf->amp,
                       n, m, b0, b1, b2, s_hi, s_mid, s_lo, state->k - m, skip_pattern, piece_bits, pb[0], pb[1], pb[2], piece);
  HIP_TRY(hipGetLastError());
  return QSIM_OK;
}

int qsim_pack_all(const qsim_chunk* src, int m, const int32_t* bits, qsim_chunk* buf, int skip_pattern, int piece, int n_pieces) {
  return slabs_all(const_cast<qsim_chunk*>(src), m, bits, buf, skip_pattern, piece, n_pieces, true, "qsim_pack_all");
}
int qsim_unpack_all(qsim_chunk* dst, int m, const int32_t* bits, const qsim_chunk* buf, int skip_pattern, int piece, int n_pieces) {
  return slabs_all(dst, m, bits, const_cast<qsim_chunk*>(buf), skip_pattern, piece, n_pieces, false, "qsim_unpack_all");
}

int qsim_swap_global_local(qsim_chunk* const* chunks, int n_chunks, const int32_t* global_bits, const int32_t* local_bits, int m) {
  if (!chunks || !global_bits || !local_bits) return fail(QSIM_ERR_INVALID, "qsim_swap_global_local: null argument");
  if (m < 1 || m > 3) return fail(QSIM_ERR_INVALID, "qsim_swap_global_local: 1..3 qubit pairs expected, got %d", m);
  if (n_chunks < 2 || (n_chunks & (n_chunks - 1)) || n_chunks > 4096)
    return fail(QSIM_ERR_INVALID, "qsim_swap_global_local: chunk count must be a power of two >= 2");
  int rc = QSIM_OK;
  for (int i = 0; i < n_chunks; ++i) {
    if ((rc = check_chunk(chunks[i], "qsim_swap_global_local"))) return rc;
    if (chunks[i]->k != chunks[0]->k || chunks[i]->device != chunks[0]->device)
      return fail(QSIM_ERR_INVALID, "qsim_swap_global_local: chunks differ in size or device");
  }
  const int k = chunks[0]->k;
  int g_bits = 0;
  while ((1 << g_bits) < n_chunks) ++g_bits;
  if ((rc = check_swapped_bits(k, g_bits, m, local_bits, global_bits, "qsim_swap_global_local", "chunks", "chunk-index bit"))) return rc;
  int sorted[3] = {0, 0, 0};
  std::copy(local_bits, local_bits + m, sorted);
  std::sort(sorted, sorted + m);
  HIP_TRY(hipSetDevice(chunks[0]->device));
  const u64 n_slab = 1ull << (k - m);
  auto local_offset = [&](int pattern) {
    u64 off = 0;
    for (int i = 0; i < m; ++i) if ((pattern >> i) & 1) off |= 1ull << local_bits[i];
    return off;
  };
  for (int c = 0; c < n_chunks; ++c) {
    int mine = 0;                                   // pattern of this chunk's swapped index bits
    for (int i = 0; i < m; ++i) mine |= ((c >> global_bits[i]) & 1) << i;
    for (int d = 0; d < (1 << m); ++d) {
      if (d == mine) continue;
      const int peer = peer_of(c, m, global_bits, d);
      if (peer < c) continue;                       // each unordered pair once
      hipLaunchKernelGGL(k_swap_slabs, dim3(stream_grid(n_slab)), dim3(kBlock), 0, chunks[0]->stream,
                         chunks[c]->amp, chunks[peer]->amp, n_slab, m, sorted[0], sorted[1], sorted[2],
                         local_offset(d), local_offset(mine));
      HIP_TRY(hipGetLastError());
    }
  }
  return QSIM_OK;
}

// The slab-storing end of an op list whose tile passes (all but a kept last one) have been queued: the out side of the split
// form (the pieces are stored by qsim_apply_ops_io_part), or the pack passes of a list that could not fuse them.
static int finish_out_side(qsim_chunk* c, const qsim_ops_io* io, const FusedIo& fio, const CachedPass* kept) {
  int rc = QSIM_OK;
  if (io->dst && io->dst_parts != 0) {
    // split form: partial launches of the kept last pass, or (nothing fusable) qsim_pack_all pieces of the final state, or
    // nothing (stored already)
    SplitIo::Out& o = split_record(c)->out;
    o = SplitIo::Out();
    o.mode = kept ? SplitIo::Out::kTile : (fio.fused_out ? SplitIo::Out::kDone : SplitIo::Out::kPack);
    o.m = io->dst_m;
    for (int i = 0; i < io->dst_m; ++i) o.bits[i] = io->dst_bits[i];
    o.dst = io->dst; o.dst_own = io->dst_own; o.own_pattern = io->own_pattern;
    o.cut = PieceCut::cut(c->k, io->dst_m, io->dst_bits, io->dst_parts);
    if (kept) { o.pass = *kept; o.cut.free_above(kept->a.h, kept->T - kTileLow); }
  } else if (io->dst && !fio.fused_out) {     // not fused: pack passes
    if ((rc = slabs_all(c, io->dst_m, io->dst_bits, io->dst, io->own_pattern, 0, 1, true, "qsim_apply_ops_io"))) return rc;
    if (io->own_pattern >= 0) {
      const uint64_t slab = 1ull << (c->k - io->dst_m);
      if ((rc = qsim_pack_bits(c, io->dst_m, io->dst_bits, io->own_pattern, io->dst_own, (uint64_t)io->own_pattern * slab))) return rc;
    }
  }
  return QSIM_OK;
}

// Op list with a re-layout fused into its ends (staging.py:136-152 SWAP lists): the FIRST fused pass reads
// the state from io->src in the slab layout of qsim_pack_all over io->src_bits (what an all-to-all left in the receive
// buffer) instead of a separate unpack pass, the LAST one stores it into io->dst in the slab layout over io->dst_bits
// (slab io->own_pattern, which stays on this rank, into io->dst_own) instead of a separate pack pass.  Whatever cannot
// be fused (bits inside a 128-B line, chunks too small for tile passes, an empty op list, a slab bit that is a tile
// bit of the last pass) is done with the slab kernels, so the result is the same in every case; *n_passes counts the
// HBM passes really made.  io->src_parts: the same steps, but the prepared passes are held, not launched, until the source
// pieces are announced (qsim_apply_ops_io_load).
int qsim_apply_ops_io(qsim_chunk* c, int n_ops, const int32_t* nq, const int32_t* qubits, const double* mats, const qsim_ops_io* io, int* n_passes) {
  int rc = validate_ops(c, n_ops, nq, qubits, mats);
  if (rc) return rc;
  if (!io) return fail(QSIM_ERR_INVALID, "qsim_apply_ops_io: io is null");
  if (io->struct_size != sizeof(qsim_ops_io))
    return fail(QSIM_ERR_INVALID, "qsim_apply_ops_io: io->struct_size is %u, this library's qsim_ops_io has %zu bytes (zero the struct, "
                "set struct_size = sizeof(qsim_ops_io) and rebuild against this library's include/qsim_hip.h)", io->struct_size, sizeof(qsim_ops_io));
  if (io->n_tiles < 0 || (io->n_tiles && !io->tile_masks)) return fail(QSIM_ERR_INVALID, "qsim_apply_ops_io: bad tile list");
  auto check_side = [&](const qsim_chunk* b, int m, const int32_t* bits, const char* side) -> int {
    int r = check_chunk(b, "qsim_apply_ops_io");
    if (r) return r;
    if (b->k != c->k || b->device != c->device || b->amp == c->amp)
      return fail(QSIM_ERR_INVALID, "qsim_apply_ops_io: the %s buffer must be a distinct chunk of the state's size and device", side);
    if (m < 1 || m > 3 || m > c->k) return fail(QSIM_ERR_INVALID, "qsim_apply_ops_io: %s: 1..3 slab bits expected, got %d", side, m);
    bool repeated;
    if (const int i = bad_slab_bit(c->k, m, bits, &repeated); i >= 0)
      return repeated ? fail(QSIM_ERR_INVALID, "qsim_apply_ops_io: %s: repeated slab bit %d", side, bits[i])
                      : fail(QSIM_ERR_NONLOCAL, "qsim_apply_ops_io: %s slab bit %d is non-local for 2^%d amplitudes", side, bits[i], c->k);
    return QSIM_OK;
  };
  if (io->src && (rc = check_side(io->src, io->src_m, io->src_bits, "source"))) return rc;
  if (io->dst) {
    if ((rc = check_side(io->dst, io->dst_m, io->dst_bits, "destination"))) return rc;
    if (io->own_pattern < -1 || io->own_pattern >= (1 << io->dst_m)) return fail(QSIM_ERR_INVALID, "qsim_apply_ops_io: own_pattern out of range");
    if (io->own_pattern >= 0 && (rc = check_side(io->dst_own, io->dst_m, io->dst_bits, "own-slab"))) return rc;
    if (io->own_pattern >= 0 && io->dst_own->amp == io->dst->amp) return fail(QSIM_ERR_INVALID, "qsim_apply_ops_io: the own-slab buffer must differ from the destination");
    if (io->src && io->src->amp == io->dst->amp)
      return fail(QSIM_ERR_INVALID, "qsim_apply_ops_io: the source buffer must differ from the destination buffer (one pass may read and write them at once)");
    // (dst_own == src is allowed: with two or more kernels the source has been consumed before the own slab is stored;
    // when ONE pass does everything the own slab goes into the chunk instead -- qsim_apply_ops_io_own_slab tells)
  }
  HIP_TRY(hipSetDevice(c->device));
  std::vector<FusedOp> ops;
  classify_ops(n_ops, nq, qubits, mats, &ops);
  const bool tiles = c->k >= kTileMinChunk && c->k <= kTileMaxQubits && !ops.empty();
  auto whole_lines = [](int m, const int32_t* bits) { for (int i = 0; i < m; ++i) if (bits[i] < kTileLow) return false; return true; };
  FusedIo fio;
  if (io->src && tiles && whole_lines(io->src_m, io->src_bits)) {
    fio.src = io->src;
    fio.in.m = io->src_m;
    for (int i = 0; i < io->src_m; ++i) fio.in.bits[i] = io->src_bits[i];
  }
  if (io->dst && tiles && whole_lines(io->dst_m, io->dst_bits)) {
    fio.dst = io->dst;
    fio.dst_own = io->dst_own;
    fio.own_pattern = io->own_pattern;
    fio.out.m = io->dst_m;
    for (int i = 0; i < io->dst_m; ++i) fio.out.bits[i] = io->dst_bits[i];
  }
  c->own_in_chunk = false;
  if (parts_pending(c))
    return fail(QSIM_ERR_INVALID, "qsim_apply_ops_io: pieces of an earlier split call are pending on this chunk (qsim_apply_ops_io_part / _load)");
  fio.parts = io->dst && io->dst_parts != 0;
  const bool defer = io->src && io->src_parts != 0;     // plan now, launch as the source pieces are announced
  std::vector<CachedPass> held;                         // prepared, not launched: every pass (defer), or the last one (kept for _part)
  int passes = 0;
  if (io->src && !fio.src) {           // not fusable: one unpack pass brings the state into the chunk (defer: piece by piece)
    if (!defer && (rc = slabs_all(c, io->src_m, io->src_bits, const_cast<qsim_chunk*>(io->src), -1, 0, 1, false, "qsim_apply_ops_io"))) return rc;
    ++passes;
  }
  if (tiles) {
    int p = 0;
    const TileHint hint = {io->tile_masks, io->n_tiles};
    rc = run_fused(c, ops, RawOps{n_ops, nq, qubits, mats}, io->n_tiles ? &hint : nullptr, &fio, &p,
                   [&](TileArgs& a, int T, double alg_bytes, bool last) {
                     if (!defer && !stays_for_parts(fio, T, last)) return dispatch_planned(c, a, T, alg_bytes);
                     held.push_back(CachedPass{a, T, alg_bytes});
                     return (int)QSIM_OK;
                   });
    if (rc) return rc;
    passes += p;
    c->own_in_chunk = fio.own_in_chunk;
    if (fio.src && !fio.fused_in) return fail(QSIM_ERR_INVALID, "internal: the first pass did not take the source buffer");
  } else {
    if (!defer && (rc = qsim_apply_ops_unfused(c, n_ops, nq, qubits, mats))) return rc;
    passes += n_ops;
  }
  if (io->dst && !fio.fused_out) ++passes;                 // a pack pass (whole, or piece by piece)
  if (defer) {
    SplitIo::In& in = split_record(c)->in;
    in = SplitIo::In();
    in.tiles = tiles;
    in.io = *io;
    in.io.tile_masks = nullptr;                             // (the caller's array: used by the plan above only)
    in.io.n_tiles = 0;
    in.fio = fio;
    in.cut = PieceCut::cut(c->k, io->src_m, io->src_bits, io->src_parts);
    // the first pass in partial launches: when it reads the source itself, is not also the slab-storing pass of a split
    // / fused destination, and the top piece bits are no tile bits of it
    const bool first_stores = held.size() == 1 && io->dst != nullptr;
    if (fio.src && !first_stores && !held.empty() && held[0].T == kTileBitsMax) in.cut.free_above(held[0].a.h, kTileBitsMax - kTileLow);
    in.passes.swap(held);
    if (!tiles) {                                           // gate by gate, once the source is complete
      in.nq.assign(nq, nq + n_ops);
      in.qubits.assign(qubits, qubits + 2 * (size_t)n_ops);
      in.mats.assign(mats, mats + 32 * (size_t)n_ops);
    }
    in.active = true;
  } else if ((rc = finish_out_side(c, io, fio, held.empty() ? nullptr : &held[0]))) {
    return rc;
  }
  c->last_passes = passes;
  if (n_passes) *n_passes = passes;
  return QSIM_OK;
}

// Split form of the slab-storing end of qsim_apply_ops_io (qsim_ops_io::dst_parts): store piece `part` of every slab.
int qsim_apply_ops_io_part(qsim_chunk* c, int part) {
  int rc = check_chunk(c, "qsim_apply_ops_io_part");
  if (rc) return rc;
  if (!c->split || c->split->out.mode == SplitIo::Out::kNone) return fail(QSIM_ERR_INVALID, "qsim_apply_ops_io_part: no split op list is pending on this chunk");
  SplitIo::Out& o = c->split->out;
  const int n_parts = o.cut.n_parts();
  if (part < 0 || part >= n_parts) return fail(QSIM_ERR_INVALID, "qsim_apply_ops_io_part: piece %d out of range", part);
  if ((o.stored >> part) & 1) return fail(QSIM_ERR_INVALID, "qsim_apply_ops_io_part: piece %d has been stored already", part);
  HIP_TRY(hipSetDevice(c->device));
  if (o.mode == SplitIo::Out::kTile) {
    // the partial launch that holds this piece: it stores 2^(nb - nb_free) pieces
    if ((rc = launch_group(c, o.pass, o.cut, o.cut.group_of(part)))) return rc;
  } else if (o.mode == SplitIo::Out::kPack) {
    // (the pieces of qsim_pack_all are the values of the top non-slab index bits: the same cut)
    if ((rc = slabs_all(c, o.m, o.bits, o.dst, o.own_pattern, part, n_parts, true, "qsim_apply_ops_io_part"))) return rc;
    if (o.own_pattern >= 0 && o.stored == 0) {              // the own slab goes to the receive buffer whole, with the first piece
      const uint64_t slab = 1ull << (c->k - o.m);
      if ((rc = qsim_pack_bits(c, o.m, o.bits, o.own_pattern, o.dst_own, (uint64_t)o.own_pattern * slab))) return rc;
    }
  }
  o.stored |= 1u << part;
  if (o.stored == (1u << n_parts) - 1u) o.mode = SplitIo::Out::kNone;
  return QSIM_OK;
}

// Receive side of the split form (qsim_ops_io::src_parts): piece `part` of every slab of the source has arrived (its
// transfer is ordered before this call on the chunk's stream).  Launches what can run: an unpack piece, a partial launch of
// the first pass whose source pieces are all there, and -- with the last piece -- everything else of the op list.
int qsim_apply_ops_io_load(qsim_chunk* c, int part) {
  int rc = check_chunk(c, "qsim_apply_ops_io_load");
  if (rc) return rc;
  if (!c->split || !c->split->in.active) return fail(QSIM_ERR_INVALID, "qsim_apply_ops_io_load: no op list with a split source is pending on this chunk");
  SplitIo::In& in = c->split->in;
  const int n_parts = in.cut.n_parts();
  if (part < 0 || part >= n_parts) return fail(QSIM_ERR_INVALID, "qsim_apply_ops_io_load: piece %d out of range", part);
  if ((in.announced >> part) & 1) return fail(QSIM_ERR_INVALID, "qsim_apply_ops_io_load: piece %d has been announced already", part);
  HIP_TRY(hipSetDevice(c->device));
  PendingGuard guard{c, true};        // an error leaves nothing pending
  in.announced |= 1u << part;
  const qsim_ops_io* io = &in.io;
  if (!in.fio.src) {                  // unpack mode: this piece goes home now
    if ((rc = slabs_all(c, io->src_m, io->src_bits, const_cast<qsim_chunk*>(io->src), -1, part, n_parts, false, "qsim_apply_ops_io_load"))) return rc;
  } else if (in.cut.nb_free > 0) {    // partial launches of the first pass: a group runs once all its pieces are there
    const int shift = in.cut.nb - in.cut.nb_free, g = in.cut.group_of(part);
    const unsigned group = ((1u << (1 << shift)) - 1u) << (g << shift);
    if ((in.announced & group) == group && (rc = launch_group(c, in.passes[0], in.cut, g))) return rc;
  }
  if (in.announced != (1u << n_parts) - 1u) { guard.armed = false; return QSIM_OK; }
  // the source is complete: the rest of the op list
  in.active = false;
  const CachedPass* kept = nullptr;
  if (in.tiles) {
    for (size_t i = 0; i < in.passes.size(); ++i) {
      if (i == 0 && in.cut.nb_free > 0) continue;           // ran in partial launches
      CachedPass& p = in.passes[i];
      if (stays_for_parts(in.fio, p.T, i + 1 == in.passes.size())) kept = &p;
      else if ((rc = dispatch_planned(c, p.a, p.T, p.alg_bytes))) return rc;
    }
  } else {
    if ((rc = qsim_apply_ops_unfused(c, (int)in.nq.size(), in.nq.data(), in.qubits.data(), in.mats.data()))) return rc;
  }
  if ((rc = finish_out_side(c, io, in.fio, kept))) return rc;
  guard.armed = false;
  return QSIM_OK;
}

// Where the last qsim_apply_ops_io on this chunk left the slab that stays on the rank: 0 = in io->dst_own, 1 = in the chunk
// itself (dst_own was the source buffer and one pass did everything; the exchange then has to deliver into the chunk).
int qsim_apply_ops_io_own_slab(const qsim_chunk* c, int32_t* in_chunk) {
  if (!c || !in_chunk) return fail(QSIM_ERR_INVALID, "qsim_apply_ops_io_own_slab: null argument");
  *in_chunk = c->own_in_chunk ? 1 : 0;
  return QSIM_OK;
}

// The pieces of one side of the pending split op list (m slab bits) and the launches its pass takes.
static int report_pieces(const qsim_chunk* c, const PieceCut& cut, int m, int launches, int32_t* n_parts, uint64_t* piece_amps, int32_t* n_launches) {
  if (n_parts) *n_parts = cut.n_parts();
  if (piece_amps) *piece_amps = cut.piece_amps(c->k, m);
  if (n_launches) *n_launches = launches;
  return QSIM_OK;
}

// Source pieces of the pending op list (qsim_ops_io::src_parts): how many, their size, and how many partial launches the
// first pass takes (0: it runs whole after the last piece).
int qsim_apply_ops_io_source_parts(const qsim_chunk* c, int32_t* n_parts, uint64_t* piece_amps, int32_t* n_launches) {
  if (!c || !c->split || !c->split->in.active) return fail(QSIM_ERR_INVALID, "qsim_apply_ops_io_source_parts: nothing pending on this chunk");
  const SplitIo::In& in = c->split->in;
  return report_pieces(c, in.cut, in.io.src_m, in.cut.nb_free > 0 ? (1 << in.cut.nb_free) : 0, n_parts, piece_amps, n_launches);
}

// The pieces of the pending split op list: piece j of EVERY slab d is [d * 2^(k - m) + j * piece_amps, + piece_amps) of the
// send / receive buffers.  n_parts depends only on (k, m, dst_parts): the same on every rank.
int qsim_apply_ops_io_parts(const qsim_chunk* c, int32_t* n_parts, uint64_t* piece_amps, int32_t* n_launches) {
  if (!c || !c->split || c->split->out.mode == SplitIo::Out::kNone) return fail(QSIM_ERR_INVALID, "qsim_apply_ops_io_parts: no split op list is pending on this chunk");
  const SplitIo::Out& o = c->split->out;
  const int launches = o.mode == SplitIo::Out::kTile ? (1 << o.cut.nb_free) : (o.mode == SplitIo::Out::kPack ? o.cut.n_parts() : 0);
  return report_pieces(c, o.cut, o.m, launches, n_parts, piece_amps, n_launches);
}
}  // extern "C"
