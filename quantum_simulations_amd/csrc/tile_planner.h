// tile_planner.h -- pass building of the fused passes: op list -> tiles -> passes (the rules, the greedy builder).
// Part of the single translation unit qsim_hip.hip (included there, in order; not a standalone header).
// Host only: a planned pass leaves through the `sink` of plan_fused; nothing here touches the device.
constexpr int kTileMinChunk = kTileThreadBits > 8 ? kTileThreadBits : 8;   // smaller chunks run gate by gate (a tile holds at least one amplitude per thread)

// Pass builder.  Ops are taken in list order; an op whose non-diagonal targets are not all tile
// bits has to wait and blocks its qubits: its TARGET qubits for every later op, its diagonal qubits (controls,
// phase bits) only for later ops that target them -- two ops that act diagonally on every qubit they share commute
// (CNOTs with a common control, a phase gate on a control, CZ / CR among themselves), so the later one may run a
// pass earlier than the one that waits; likewise ops that act as 1 or X on a shared qubit (CNOTs with a common
// target, X on a CNOT target) (round 3: 155 -> 148 passes over 8 random circuits at 28 qubits, 93 -> 84
// over 6 Clifford+T circuits, 21 -> 20 on the 30-qubit bench circuit; tuning().plan_commute).  Ops on disjoint
// qubits commute anyway; everything else keeps its list order.  WHICH qubits become the tile's
// high bits decides how many ops a pass holds:
//   * first come: an op that still fits claims the bits it needs (the only rule up to r01e);
//   * look-ahead: starting from the first 0, 2, 4, 6 of those bits, add the bit that lets the pass
//     hold the most ops, one at a time;
// the candidate that holds the most ops wins (first come on ties).  On the 28-qubit bench circuit
// this needs 20-21 passes instead of 24 (tests/test_tile_planner_cpu.py); the search costs about
// 0.3 ms per pass on the host, hidden behind the previous pass on the device for large states and
// switched off for small ones; from 26 qubits on each candidate is also scored by what the pass
// AFTER it could hold (one pass fewer on the bench circuits).  QSIM_PLAN_LOOKAHEAD = 0 / 1 / 2 forces.
// `sink(args, T, algorithmic_bytes, first, last)` receives every planned pass (first / last of the op list): the
// launcher on the device path, a serialiser in qsim_plan_ops (the planner itself never touches the GPU).
// `hint` (qsim_apply_ops_tiled): the caller names the high tile bits of the first passes itself -- a host that has planned
// the list once and moved its qubits to other index bits (a layout chosen for the memory pattern of the tiles:
// runner/engine.py) gets the SAME passes on the new bits instead of whatever the search finds there.  A hint that holds no
// op (or too many bits) is ignored and the search takes over for that pass.  `earliest` (qsim_apply_ops_placed; optional, one
// entry per op of the planned list): op i does not run before pass earliest[i] of the named passes -- in an earlier pass
// it waits like an op whose target is not in the tile, and blocks what depends on it, so ANY values give a correct
// program.  It is how a host that has priced the passes (qsim_plan_balance) moves ops that need no tile out of a pass
// whose gate engine is the bottleneck into a later one that has room.  Ignored from the first pass the hint does not name.
struct TileHint { const uint64_t* masks; int n; const int32_t* earliest = nullptr; };
// Peek mode (qsim_plan_peek_pass, the partition planner of runner/partition_plan.py): the op list lives on `n_total` >= k
// index bits; the bits >= k are RANK bits of a partitioned state -- never tile bits, never targets (an op that targets one
// waits, and blocks like any waiting op), but fine as controls and phase bits (a rank applies or skips such an op by its own
// rank bits).  `done` marks the ops that ran already; the builder chooses the tile of the NEXT pass exactly as it would in a
// full plan (candidates, look-ahead), reports it with its members and stops: nothing is emitted.
struct PeekPlan {
  int n_total;
  const uint8_t* done;         // per op of ops_in
  uint64_t avoid;              // index bits the tile should not hold unless its ops need them (the slab bits of a coming re-layout)
  uint64_t tile_mask;          // out: high tile bits (with the fill)
  uint64_t need_mask;          // out: ... of which the pass's ops need
  std::vector<size_t>* members;  // out: indices into ops_in
};

// The rules of pass building, one copy for the greedy builder (plan_fused) and the searching one (tile_search.h): which ops
// a tile holds (`holds`), which tiles are worth trying (`candidates`, `grow`), what a tile costs in memory pattern
// (`conflicts`) and what a pass on a tile really emits (`emit`).  The state is the done-set of the op list; `begin_pass`
// brings the scan bounds up to date with it.
struct PassBuilder {
  const Tuning& tune;
  const std::vector<FusedOp>& ops;
  const int k, T, low, cap;                    // cap: tile high-bit capacity
  const size_t n_ops;
  std::vector<char> done;
  std::vector<u64> qm, need;                   // all qubits of an op; its target bits above the low bits
  std::vector<u64> tm;                         // the qubits an op acts on NON-diagonally (its targets); qm & ~tm: controls, phase bits
  std::vector<u64> xm;                         // ... of those, the ones it acts on as 1 or X only (X, CNOT targets): X-diagonal
  u64 all_qubits, rank_bits;                   // (rank bits: peek mode only: no tile bit, no target)
  bool lookahead;
  const int32_t* earliest = nullptr;           // TileHint::earliest while the hint names the pass, and the pass being built
  int pass_no = 0;
  size_t remaining, first = 0;
  // How far behind `first` a pass looks for ops (counted in ops not yet done).  The scans below end early once every
  // qubit is blocked for everything (`bt`), which never happens while some qubit is used only as a control, phase bit or
  // X target (a GHZ root, a phase-estimation ancilla, an idle qubit): every scan then walked the whole remaining list --
  // 12 ms of host planning per pass on a 4000-op list, several times the device time of the pass.  An op
  // that far behind the front has a few thousand waiting ops on at most 35 qubits in front of it and is admissible only
  // by accident; it runs a pass later.  Lists shorter than the window (the bench circuits, QFT(33)) plan as before.
  // (byte-identical plans to the unbounded scan on the 28- / 30-qubit bench and Clifford+T circuits from 384 on; lists
  // of more than four windows use two thirds of it: 7.5 -> 1.4 ms per pass on a 4000-op list with a control-only qubit)
  int scan_window;
  // What a pass costs (round 19, runner/engine_cost_model.json, profiles/r19a_pass_engine_split.txt): max(memory time of its
  // tile, 0.68 ms + its records), a record 12 (Z) .. 27 (real 2x2) .. 57 us (complex 2x2) at 28 qubits, a group change 44 us.
  // With tiles of 1.33-1.73 ms a pass is memory bound up to 32-52 records of the bench mix (20 us on average) and bound by
  // the gate engine beyond -- which 7 of the 13 passes of the bench plan measurably are.  Records are therefore never free, but a
  // pass more costs what 65 of them cost, so holding more ops keeps paying up to the record budget: kSaturated is no
  // knee of the hardware.  It is the count from which a first-come pass is kept without looking for a fuller tile
  // (phase-heavy circuits: QFT) and the cap of the look-ahead scores, and it stays at the value the plans of the tests and
  // of profiles/ were made with; the engine time itself is priced after the search (tile_search.h plan_balance).
  static constexpr int kSaturated = 64;
  bool tie_break;                              // plan_conflict_cost = -1: conflicts only break ties between tiles that hold the same number of ops
  u64 jit_state;
  u64 forced_static = 0;                       // (probe) bits that every tile holds
  // Anchored tiles (tuning().plan_anchor = s > 0, evaluation knob of round 4): every tile after the first shares at
  // least s of its high bits with the tile of the pass before it (`prev`): those s qubits can stay on the physical
  // positions next to the line bits (2^(s+7)-byte contiguous pieces per tile, the fast DRAM pattern) while the pass's
  // store permutes the tile's qubits among the tile's positions.  The carried bits are grown greedily from the
  // previous tile (the bit that lets the pass hold the most ops, one at a time).
  int anchor;
  std::vector<u64> cands, cands2;              // scratch of choose_tile
  std::vector<size_t> trial;

  PassBuilder(int k_, const std::vector<FusedOp>& ops_, int n_bits)
      : tune(tuning()), ops(ops_), k(k_), T(k_ < kTileBitsMax ? k_ : kTileBitsMax), low(kTileLow), cap(T - kTileLow),
        n_ops(ops_.size()), done(ops_.size(), 0), qm(ops_.size()), need(ops_.size()), tm(ops_.size()), xm(ops_.size()) {
    for (size_t i = 0; i < n_ops; ++i) {
      qm[i] = op_qmask(ops[i]);
      need[i] = 0;
      tm[i] = xm[i] = 0;
      for (int t = 0; t < ops[i].ntargets; ++t) {
        tm[i] |= 1ull << ops[i].target[t];
        if (ops[i].target[t] >= low) need[i] |= 1ull << ops[i].target[t];
      }
      if (ops[i].kind == TG_SWAP1 && tune.plan_commute >= 2) xm[i] = tm[i];
      if (!tune.plan_commute) tm[i] = qm[i];     // (off: every qubit of a waiting op blocks everything on it)
    }
    all_qubits = n_bits >= 64 ? ~0ull : ((1ull << n_bits) - 1);
    rank_bits = all_qubits & ~(k >= 64 ? ~0ull : ((1ull << k) - 1));
    lookahead = tune.plan_lookahead >= 0 ? tune.plan_lookahead != 0 : k >= 24;
    remaining = n_ops;
    scan_window = tune.plan_scan_window;
    tie_break = tune.plan_conflict_cost < 0;
    jit_state = 0x9E3779B97F4A7C15ull * (u64)(tune.plan_jitter + 1);
    for (int b = low; b < low + tune.plan_force_low && b < k && __builtin_popcountll(forced_static) < cap; ++b) forced_static |= 1ull << b;
    anchor = tune.plan_anchor;
  }

  // Two ops commute when each acts diagonally on every qubit they share (CNOTs with a common control, a phase gate on
  // a control, CZ / CR among themselves ...) -- or, plan_commute >= 2, both as 1 / X (CNOTs with a common target, X on a
  // CNOT target).  An op that has to wait therefore blocks its general TARGET qubits for everything, its diagonal
  // qubits for ops that target them and its X-type targets for everything but X-type targets:
  // `bt` = qubits blocked for all, `bd` = blocked for targets, `bx` = blocked for all but X-type targets.
  struct Blocked {
    const PassBuilder& pb;
    u64 bt = 0, bd = 0, bx = 0;
    bool admits(size_t i) const { return !(pb.qm[i] & bt) && !(pb.tm[i] & bd) && !((pb.qm[i] & ~pb.xm[i]) & bx); }
    bool add(size_t i) {                       // op i waits; true: every qubit is now blocked for everything
      bt |= pb.tm[i] & ~pb.xm[i];
      bx |= pb.xm[i];
      bd |= pb.qm[i] & ~pb.tm[i];
      return bt == pb.all_qubits;
    }
  };

  // the scan bounds of the next pass, from the done-set
  void begin_pass() {
    while (first < n_ops && done[first]) ++first;
    scan_window = remaining > 4 * (size_t)tune.plan_scan_window ? std::max(1, tune.plan_scan_window * 2 / 3) : tune.plan_scan_window;
  }

  // ops a pass with the given high bits would hold (optionally listed)
  int holds(u64 tile_mask, std::vector<size_t>* out) const {
    Blocked blocked{*this};
    int count = 0, seen = 0;
    for (size_t i = first; i < n_ops && count < tune.max_gates_per_pass; ++i) {
      if (done[i]) continue;
      if (++seen > scan_window) break;
      if (!blocked.admits(i) || (need[i] & ~tile_mask) || (earliest && earliest[i] > pass_no)) {
        if (blocked.add(i)) break;
        continue;
      }
      ++count;
      if (out) out->push_back(i);
    }
    return count;
  }
  // Memory pattern of a tile (profiles/r02z_tile_bits_samples.txt, 2500 gate-less passes): index bits b and b + 7
  // with b = 13..16 in ONE tile cost +0.13-0.17 ms each at 28 qubits (+9 %; byte-address bits 17-20 select the
  // bank, 24-27 are row bits folded into it: both varying inside a tile puts two rows on one bank), bits 18 / 26 and
  // 19 / 27 half of that.  Counted in units of ops a pass holds (tuning().plan_conflict_cost each).
  static int conflicts(u64 mask) {
    int c = 0;
    for (int b = 13; b <= 16; ++b) c += 2 * (int)(((mask >> b) & (mask >> (b + 7)) & 1));
    for (int b = 18; b <= 19; ++b) c += (int)(((mask >> b) & (mask >> (b + 8)) & 1));
    return c;
  }
  int penalty(u64 mask) const { return tune.plan_conflict_cost > 0 ? tune.plan_conflict_cost * conflicts(mask) / 2 : 0; }
  // (the fitted per-bit + pair model of the same samples as the tie-break instead of the conflict count: 159 instead of
  // 155 passes over 8 circuits, +2.3 % time -- breaking every tie perturbs the greedy growth more than it saves)
  unsigned jitter() { jit_state ^= jit_state << 13; jit_state ^= jit_state >> 7; jit_state ^= jit_state << 17; return (unsigned)(jit_state >> 33); }
  int keyed(int count, u64 mask) {
    if (tune.plan_jitter > 0) return (count - (int)(jitter() % 8 == 0) - (int)(jitter() % 16 == 0)) * 64 + (int)(jitter() % 64);
    return tie_break ? count * 64 - conflicts(mask) : count;
  }
  static u64 mask_of(const std::vector<int>& bits, size_t n) { u64 m = 0; for (size_t i = 0; i < n && i < bits.size(); ++i) m |= 1ull << bits[i]; return m; }

  // look-ahead growth of a tile: add the bit that lets the pass hold the most ops, one at a time, up to a whole tile
  // (grow_memo, the searching builder only: it grows some sixty tiles from one done-set, which end in about nine -- their
  // paths meet, and from a mask that an earlier path went through the growth is the same, so its end is taken from there.
  // Exact while the choice of a bit depends on the mask and the done-set alone, that is without the jitter probe; whoever
  // switches it on clears it whenever `done`, `first`, the scan window or the placement change.)
  bool grow_memo_on = false;
  std::vector<std::pair<u64, u64>> grow_memo;  // a mask a growth went through -> where that growth ended
  u64 grow(u64 mask) {
    const bool memo = grow_memo_on && tune.plan_jitter <= 0;
    const size_t known = grow_memo.size();
    std::vector<u64> path;
    while (__builtin_popcountll(mask) < cap) {
      if (memo) {
        size_t at = 0;
        while (at < known && grow_memo[at].first != mask) ++at;
        if (at < known) { mask = grow_memo[at].second; break; }
        path.push_back(mask);
      }
      int pick = -1, pick_count = -(1 << 20);
      for (int b = low; b < k; ++b) {
        if ((mask >> b) & 1) continue;
        const int c = keyed(holds(mask | (1ull << b), nullptr) - penalty(mask | (1ull << b)), mask | (1ull << b));
        if (c > pick_count) { pick_count = c; pick = b; }
      }
      if (pick < 0) break;
      mask |= 1ull << pick;
    }
    for (u64 through : path) grow_memo.push_back({through, mask});
    return mask;
  }

  // first come: an op that still fits claims the bits it needs (`claimed`: in that order); returns the tile
  u64 first_come(u64 forced, std::vector<int>* claimed) const {
    const int n_forced = __builtin_popcountll(forced);
    Blocked blocked{*this};
    u64 mask = forced;
    int count = 0, seen = 0;
    for (size_t i = first; i < n_ops && count < tune.max_gates_per_pass; ++i) {
      if (done[i]) continue;
      if (++seen > scan_window) break;
      bool ok = blocked.admits(i);
      const u64 extra = need[i] & ~mask;
      if (ok && (n_forced + (int)claimed->size() + __builtin_popcountll(extra) > cap || (extra & rank_bits))) ok = false;
      if (!ok) { if (blocked.add(i)) break; continue; }
      for (u64 e = extra; e; e &= e - 1) claimed->push_back(__builtin_ctzll(e));
      mask |= extra;
      ++count;
    }
    return mask;
  }

  // candidate tiles for the next pass from the current `done` / `first`: [0] = first come, then the
  // look-ahead ones grown from the first `seed` claimed bits (`always`: also where the greedy builder does without
  // the look-ahead, small states)
  void candidates(std::vector<u64>* out, size_t max_seed, size_t seed_step, u64 prev, bool always = false) {
    u64 forced = forced_static;
    if (anchor > 0 && prev) {
      for (int picked = 0; picked < anchor && picked < cap; ++picked) {
        int pick = -1, pick_count = -(1 << 20);
        for (int b = low; b < k; ++b) {
          if (!((prev >> b) & 1) || ((forced >> b) & 1)) continue;
          const int c = holds(forced | (1ull << b), nullptr);
          if (c > pick_count) { pick_count = c; pick = b; }
        }
        if (pick < 0) break;
        forced |= 1ull << pick;
      }
    }
    std::vector<int> claimed;                   // high bits in the order they were claimed
    first_come(forced, &claimed);
    out->clear();
    out->push_back(forced | mask_of(claimed, claimed.size()));
    if (!((lookahead || always) && k - low > cap) || holds(out->front(), nullptr) >= kSaturated) return;
    for (size_t seed = 0; seed <= max_seed && seed <= claimed.size(); seed += seed_step)
      out->push_back(grow(forced | mask_of(claimed, seed)));
  }

  // the high bits of a tile mask, filled with the lowest unused bits so the tile always has T bits (bits 3.. conflict
  // with nothing), ascending
  std::vector<int> filled(std::vector<int> high) const {
    for (int b = low; (int)high.size() < cap && b < k; ++b)
      if (std::find(high.begin(), high.end(), b) == high.end()) high.push_back(b);
    std::sort(high.begin(), high.end());
    return high;
  }
  std::vector<int> bits_of(u64 mask) const {
    std::vector<int> high;
    for (int b = low; b < k; ++b) if ((mask >> b) & 1) high.push_back(b);
    return high;
  }

  // The register groups of one pass: `members` on the tile `high`; emitted[mi]: member mi got its records (the others did
  // not fit the record budget and wait for the next pass).
  void emit(const std::vector<size_t>& members, const std::vector<int>& high, std::vector<TileGroup>* groups, std::vector<char>* emitted) const {
    emitted->assign(members.size(), 0);
    GroupEmitter::emit(ops, members, high, T, groups, emitted);
    if (lookahead && tune.tile_direct && tune.tile_last_search && T == kTileBitsMax) {
      // second plan of the same pass with the last group chosen from the end (GroupEmitter::reserve_last); LDS round trips of a
      // tile = group changes + a first group that is not loaded in place + a last group that is not stored in place
      auto trips = [&](const std::vector<TileGroup>& g) {
        return g.empty() ? 1 << 20 : (int)g.size() + (g.front().s[0] < kTileLow) + (g.back().s[0] < kTileLow);
      };
      auto count = [](const std::vector<char>& e) { size_t c = 0; for (char x : e) c += x != 0; return c; };
      std::vector<char> emitted2(members.size(), 0);
      std::vector<TileGroup> groups2;
      GroupEmitter::emit(ops, members, high, T, &groups2, &emitted2, true);
      if (count(emitted2) > count(*emitted) || (count(emitted2) == count(*emitted) && trips(groups2) < trips(*groups))) {
        groups->swap(groups2);
        emitted->swap(emitted2);
      }
      // (four more variants -- the first group's preference for a direct triple off / stronger, each with and without the
      // last-group search -- save one more round trip in 84 on the bench circuit: not worth three times the planning)
    }
  }

  // The tile of the next pass: the caller's hint when it holds an op; else the candidate that holds the most ops
  // (first come on ties), from 26 qubits on (`depth2`) also scored by what the pass AFTER it could hold.
  u64 choose_tile(const TileHint* hint, int pass, u64 prev_mask, bool depth2) {
    if (hint && pass < hint->n) {
      const u64 m = hint->masks[pass] & all_qubits & ~((1ull << low) - 1);
      if (m && __builtin_popcountll(m) <= cap && holds(m, nullptr) > 0) return m;
    }
    candidates(&cands, 6, 2, prev_mask);
    u64 best_mask = cands[0];
    int best_score = -(1 << 20);
    for (size_t ci = 0; ci < cands.size(); ++ci) {
      trial.clear();
      int score = std::min(holds(cands[ci], &trial), kSaturated) - penalty(cands[ci]);
      if (depth2 && cands.size() > 1 && trial.size() < remaining) {
        // what the pass AFTER this one could hold (a smaller candidate set)
        const size_t first_saved = first;
        for (size_t i : trial) done[i] = 1;
        while (first < n_ops && done[first]) ++first;
        candidates(&cands2, 4, 4, cands[ci]);
        int next_best = 0;
        for (u64 m2 : cands2) next_best = std::max(next_best, std::min(holds(m2, nullptr), kSaturated) - penalty(m2));
        for (size_t i : trial) done[i] = 0;
        first = first_saved;
        score += next_best;
      } else if (depth2 && trial.size() >= remaining) {
        score += 2 * kSaturated;                // finishes the list
      }
      score = keyed(score, cands[ci]);
      if (score > best_score) { best_score = score; best_mask = cands[ci]; }
    }
    return best_mask;
  }

  // peek mode: of the tile `high` only the bits its members need are kept, and the fill leaves out the bits to avoid;
  // returns the needed bits
  u64 keep_needed(const std::vector<size_t>& members, u64 avoid, std::vector<int>* high) const {
    u64 needed = 0;
    for (size_t i : members) needed |= need[i];
    std::vector<int> kept;
    for (int b : *high) if ((needed >> b) & 1) kept.push_back(b);
    for (int b = low; (int)kept.size() < cap && b < k; ++b)                        // the fill: not the bits to avoid
      if (!((avoid >> b) & 1) && std::find(kept.begin(), kept.end(), b) == kept.end()) kept.push_back(b);
    *high = kept;
    return needed;
  }
  // The members that got their records are done; returns their algorithmic bytes (dense 32N, diagonal /
  // controlled / SWAP 16N, CZ/CR 8N) and counts them.
  double account(const std::vector<size_t>& members, const std::vector<char>& emitted, size_t* n_emitted) {
    double alg_bytes = 0;
    *n_emitted = 0;
    for (size_t mi = 0; mi < members.size(); ++mi)
      if (emitted[mi]) {
        const FusedOp& o = ops[members[mi]];
        const int halvings = o.kind == TG_PHASE ? o.nbits : (o.control >= 0 ? 1 : o.halvings);
        alg_bytes += 32.0 * (double)((1ull << k) >> halvings) + 32.0 * (double)(1ull << k) * o.absorbed;
        done[members[mi]] = 1; --remaining; ++*n_emitted;
      }
    return alg_bytes;
  }
};

// ---- probes (tools/): memory-pattern and engine-floor passes with WRONG results; empty in the product library ---------
#ifdef QSIM_PROBES
static std::vector<int> probe_int_list(const char* name) {   // "b0,b1,..." from the environment
  std::vector<int> bits;
  if (const char* e = getenv(name))
    for (const char* p = e; *p;) { bits.push_back(atoi(p)); while (*p && *p != ',') ++p; if (*p) ++p; }
  return bits;
}
#endif
// tuning().debug_skip_gates = 2 / 3 / 4: the pass's tile is replaced
static void probe_tile_bits(int k, int low, int cap, std::vector<int>* high_io) {
#ifdef QSIM_PROBES
  std::vector<int>& high = *high_io;
  const int mode = tuning().debug_skip_gates;
  if (mode == 2) for (int j = 0; j < cap; ++j) high[j] = low + j;   // contiguous tiles (floor probe)
  if (mode == 3) for (int j = 0; j < cap; ++j) high[j] = k - cap + j; // far-strided tiles
  if (mode == 4) {   // tile bits from QSIM_DEBUG_TILE_BITS="b0,b1,..." (memory-pattern probe)
    const std::vector<int> bits = probe_int_list("QSIM_DEBUG_TILE_BITS");
    if ((int)bits.size() == cap) { high = bits; std::sort(high.begin(), high.end()); }
  }
#endif
}
// tuning().debug_skip_gates: profiling aid: load -> LDS -> store only
static void probe_strip_gates(std::vector<TileGroup>* groups) {
#ifdef QSIM_PROBES
  if (tuning().debug_skip_gates) {
    groups->resize(1);
    (*groups)[0].gates.clear();
  }
#endif
}
// Engine-floor probe: QSIM_DEBUG_REMAP_TILE="b0,...,b7" keeps the pass's record stream but moves
// its tile to these index bits (j-th smallest tile bit -> j-th listed bit), i.e. the same gates on another
// memory pattern: what would the pass cost if its tile always had the fastest layout?
static void probe_remap_tile(int T, int cap, TileArgs* a) {
#ifdef QSIM_PROBES
  std::vector<int> bits = probe_int_list("QSIM_DEBUG_REMAP_TILE");
  if ((int)bits.size() == cap && T == kTileBitsMax) {
    std::sort(bits.begin(), bits.end());
    uint8_t map[64];
    for (int b = 0; b < 64; ++b) map[b] = (uint8_t)b;
    for (int j = 0; j < cap; ++j) map[a->h[j]] = (uint8_t)bits[(size_t)j];
    for (int j = 0; j < cap; ++j) { a->lay_in[j] = map[a->lay_in[j]]; a->lay_out[j] = map[a->lay_out[j]]; }
    for (int j = 0; j < cap; ++j) a->h[j] = (uint8_t)bits[(size_t)j];
  }
#endif
}

// The greedy builder: one tile per pass, never revisited.  Each turn of the loop: choose the tile, list its members,
// (peek mode: report and stop), emit the register groups, account for what was emitted, serialise, hand over to `sink`.
template <class Sink>
static int plan_fused(int k, const std::vector<FusedOp>& ops_in, int* n_passes, Sink&& sink, const TileHint* hint = nullptr,
                      PeekPlan* peek = nullptr) {
  const Tuning& tune = tuning();
  const std::vector<FusedOp> ops = planned_ops(ops_in);
  PassBuilder pb(k, ops, peek ? peek->n_total : k);
  const int T = pb.T;
  *n_passes = 0;
  if (peek) {
    pb.remaining = 0;
    for (size_t i = 0; i < pb.n_ops; ++i) { pb.done[i] = peek->done[i] != 0; pb.remaining += !pb.done[i]; }
    peek->tile_mask = peek->need_mask = 0;
    peek->members->clear();
  }
  const bool depth2 = tune.plan_lookahead >= 0 ? tune.plan_lookahead >= 2 : k >= 26;
  u64 prev_mask = 0;                            // high bits of the pass before (anchored tiles)
  while (pb.remaining) {
    pb.begin_pass();
    pb.pass_no = *n_passes;
    pb.earliest = (hint && hint->earliest && *n_passes < hint->n && !tune.tile_commute_fuse) ? hint->earliest : nullptr;
    u64 best_mask = pb.choose_tile(hint, *n_passes, prev_mask, depth2);
    std::vector<size_t> members;
    pb.holds(best_mask, &members);
    if (members.empty() && pb.earliest) {          // everything admissible was told to wait: the pass is built without that
      pb.earliest = nullptr;
      best_mask = pb.choose_tile(hint, *n_passes, prev_mask, depth2);
      pb.holds(best_mask, &members);
    }
    std::vector<int> high = pb.bits_of(best_mask);   // chosen high bits
    if (peek) {
      // (everything that is left may be waiting for a rank bit: an empty pass is an answer here, not an error)
      if (members.empty()) { *n_passes = 0; return QSIM_OK; }
      peek->need_mask = pb.keep_needed(members, peek->avoid, &high);
    }
    if (members.empty()) return fail(QSIM_ERR_INVALID, "internal: fused planner made no progress");
    high = pb.filled(high);
    prev_mask = PassBuilder::mask_of(high, high.size());
    probe_tile_bits(k, pb.low, pb.cap, &high);
    TileArgs a;
    std::memset(&a, 0, sizeof a);
    a.T = T;
    for (size_t j = 0; j < high.size(); ++j) a.h[j] = (uint8_t)high[j];
    std::vector<char> emitted;
    std::vector<TileGroup> groups;
    pb.emit(members, high, &groups, &emitted);
    size_t n_emitted = 0;
    const double alg_bytes = pb.account(members, emitted, &n_emitted);
    if (!n_emitted) return fail(QSIM_ERR_INVALID, "internal: fused planner emitted nothing");
    if (peek) {
      // the ops whose records fit the pass (a rank runs this list without the ops its rank bits switch off and with the
      // rank-bit predicates gone: never more records than counted here)
      for (int b : high) peek->tile_mask |= 1ull << b;
      for (size_t mi = 0; mi < members.size(); ++mi) if (emitted[mi]) peek->members->push_back(members[mi]);
      *n_passes = 1;
      return QSIM_OK;
    }
    probe_strip_gates(&groups);
    int rc = serialize_pass(groups, &a);
    if (rc) return rc;
    probe_remap_tile(T, pb.cap, &a);
    if (tune.debug_stats) {
      size_t descs = 0;
      for (const TileGroup& g : groups) descs += g.gates.size();
      std::fprintf(stderr, "[qsim] pass %d: %zu gates, %zu groups, %zu descriptors\n", *n_passes, n_emitted, groups.size(), descs);
    }
    rc = sink(a, T, alg_bytes, *n_passes == 0, pb.remaining == 0);
    if (rc) return rc;
    ++*n_passes;
  }
  return QSIM_OK;
}
