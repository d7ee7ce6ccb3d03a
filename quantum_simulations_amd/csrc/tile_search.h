// tile_search.h -- the searching pass builder: a beam search over the tiles of an op list's fused passes.
// Part of the single translation unit qsim_hip.hip (included there, in order; not a standalone header).
//
// The greedy builder (plan_fused) chooses one tile per pass and never revisits a choice.  This one keeps `beam` partial
// plans alive per pass: a state is the done-set of the op list (plus the tiles that led to it), every state is expanded by
// a wider candidate set than the greedy builder's, states with the same done-set are merged, and the `beam` states that
// rank best (ops done, and what the next pass could do) go on to the next pass.  The first depth at which a state finishes
// the list is the pass count.
// Rules, candidates and the effect of a pass are PassBuilder's (tile_planner.h): a child's done-set is what
// PassBuilder::emit writes records for, not what holds() promises, so the tiles replay through the hint path of plan_fused
// (qsim_plan_ops_tiled, qsim_apply_ops_tiled) into exactly the passes counted here.  Host only; a few hundred times the
// greedy builder's time, for plans that run many times (runner/engine.py).
struct SearchNode { int parent; u64 mask; };     // a kept state's tile and the node of the depth before it came from
struct SearchState {
  std::vector<char> done;
  size_t remaining;
  int parent;                  // node of the state it was expanded from (-1: the start)
  u64 mask;                    // the tile of its last pass
  long rank;                   // smaller is better (see the beam cut)
  int conflicts;               // PassBuilder::conflicts summed over its tiles
  u64 hash;                    // of the done-set
};

constexpr int kSearchBeamDefault = 8;
constexpr size_t kSearchPairSeeds = 10;
constexpr int kSearchBeamMax = 4096;

// A search that runs next to others (plan_search_triples): `best` is the fewest passes any of them has reached so far.  A
// search that can no longer reach it stops and says so (`cut`) -- its result would have been thrown away -- and a search
// that can is not touched, so what survives does not depend on when `best` fell.  need_bits: the beam is also cut where
// its states cannot finish in time by the tile bits their remaining ops still need (SearchState lower bound, below).
struct SearchBound {
  const std::atomic<int>* best;
  bool need_bits;
  bool cut;                    // out: more passes than *best; masks and n_passes are the greedy plan's, not a result
};

// The tiles of the greedy plan (or of the replay of `hint`): the fall-back and the bar the search has to clear.
static int planned_tiles(int k, const std::vector<FusedOp>& ops, const TileHint* hint, std::vector<u64>* masks, int* n_passes) {
  masks->clear();
  return plan_fused(k, ops, n_passes, [&](TileArgs& a, int T, double, bool, bool) {
    u64 m = 0;
    for (int j = 0; j < T - kTileLow; ++j) m |= 1ull << a.h[j];
    masks->push_back(m);
    return (int)QSIM_OK;
  }, hint);
}

// Tiles (high-bit masks, whole tiles) of a plan of `ops_in` on k index bits with as few passes as the search finds: never
// more than the greedy builder's, whose tiles are returned when the search does not beat them.
static int plan_search(int k, const std::vector<FusedOp>& ops_in, int beam, std::vector<u64>* masks, int* n_passes,
                       SearchBound* bound = nullptr) {
  if (bound) bound->cut = false;
  beam = std::max(1, std::min(beam > 0 ? beam : kSearchBeamDefault, kSearchBeamMax));
  int rc = planned_tiles(k, ops_in, nullptr, masks, n_passes);
  if (rc) return rc;
  const int greedy_passes = *n_passes;
  const std::vector<FusedOp> ops = planned_ops(ops_in);
  PassBuilder pb(k, ops, k);
  if (greedy_passes <= 1 || k - pb.low <= pb.cap) return QSIM_OK;      // (one tile holds every qubit: nothing to choose)
  const size_t n_ops = pb.n_ops;
  pb.grow_memo_on = true;

  std::vector<std::vector<SearchNode>> nodes;    // per depth: the kept states' tiles
  std::vector<SearchState> states(1), children;
  states[0].done.assign(n_ops, 0);
  states[0].remaining = n_ops;
  states[0].parent = -1;
  states[0].mask = 0;
  states[0].conflicts = 0;
  std::vector<u64> cands, tried, seeds;
  std::vector<size_t> members, order;
  std::vector<int> claimed;
  std::vector<char> emitted;
  std::vector<TileGroup> groups;
  int finished = -1;                             // node of the last depth that finishes the list
  // (a plan of greedy_passes passes is known: the search only looks for shorter ones)
  for (int depth = 0; depth + 1 < greedy_passes && finished < 0 && !states.empty(); ++depth) {
    // The bound: every state here has run `depth` passes and needs one more at least -- with need_bits, as many as it
    // takes to bring every tile bit its remaining ops need into a tile, `cap` per pass.  Once that is past `best`, and the
    // greedy plan is too, nothing this search can still return reaches `best`.
    if (bound) {
      int more = 1;
      if (bound->need_bits) {
        more = 1 << 20;
        for (const SearchState& s : states) {
          u64 needed = 0;
          for (size_t i = 0; i < n_ops; ++i) if (!s.done[i]) needed |= pb.need[i];
          more = std::min(more, std::max(1, (__builtin_popcountll(needed) + pb.cap - 1) / pb.cap));
        }
      }
      const int best = bound->best->load(std::memory_order_relaxed);
      if (greedy_passes > best && depth + more > best) { bound->cut = true; return QSIM_OK; }
    }
    children.clear();
    for (size_t si = 0; si < states.size(); ++si) {
      const SearchState& s = states[si];
      pb.done = s.done;
      pb.remaining = s.remaining;
      pb.first = 0;
      pb.begin_pass();
      pb.grow_memo.clear();                         // (growths are shared between the candidates of ONE state)
      // Candidates: the greedy builder's first-come tile and its look-ahead tiles, grown from EVERY prefix of the
      // first-come bits; then, for every op at the front of the list (nothing undone in front of it on its qubits), the
      // tile grown around its targets -- the tiles a first-come scan never starts from.
      pb.candidates(&cands, (size_t)pb.cap, 1, s.mask, true);
      {
        PassBuilder::Blocked blocked{pb};           // (every op scanned blocks what follows it, admitted or not)
        int seen = 0;
        seeds.clear();
        for (size_t i = pb.first; i < n_ops; ++i) {
          if (pb.done[i]) continue;
          if (++seen > pb.scan_window) break;
          if (blocked.admits(i) && pb.need[i] && __builtin_popcountll(pb.need[i]) <= pb.cap &&
              std::find(seeds.begin(), seeds.end(), pb.need[i]) == seeds.end())
            seeds.push_back(pb.need[i]);
          if (blocked.add(i)) break;
        }
        for (u64 seed : seeds) cands.push_back(pb.grow(seed));
        // ... and around the targets of every two of the first kSearchPairSeeds of them (one op's targets leave most of a
        // tile to the greedy growth, which then fills it the same way from many starts: 16 passes for the 28-qubit bench
        // circuit on 1 of 48 line-qubit triples without the pairs, on 10 with them)
        for (size_t a = 0; a < seeds.size() && a < kSearchPairSeeds; ++a)
          for (size_t b = a + 1; b < seeds.size() && b < kSearchPairSeeds; ++b)
            if (__builtin_popcountll(seeds[a] | seeds[b]) <= pb.cap) cands.push_back(pb.grow(seeds[a] | seeds[b]));
      }
      tried.clear();
      for (u64 cand : cands) {
        const std::vector<int> high = pb.filled(pb.bits_of(cand));
        u64 mask = 0;
        for (int b : high) mask |= 1ull << b;
        if (std::find(tried.begin(), tried.end(), mask) != tried.end()) continue;
        tried.push_back(mask);
        members.clear();
        if (pb.holds(mask, &members) == 0) continue;
        pb.emit(members, high, &groups, &emitted);
        SearchState c;
        c.done = s.done;
        c.remaining = s.remaining;
        for (size_t mi = 0; mi < members.size(); ++mi)
          if (emitted[mi]) { c.done[members[mi]] = 1; --c.remaining; }
        if (c.remaining == s.remaining) continue;
        c.parent = depth == 0 ? -1 : (int)si;     // (states[si] is node si of the depth before)
        c.mask = mask;
        c.conflicts = s.conflicts + PassBuilder::conflicts(mask);
        c.hash = fnv1a(reinterpret_cast<const unsigned char*>(c.done.data()), n_ops);
        children.push_back(std::move(c));
      }
    }
    // Rank: the ops left, twice, less what a first-come pass could do next (a state that has done two ops fewer but
    // leaves a full pass in reach is the better one) -- 39 instead of 31 of 48 line-qubit triples of the bench circuit
    // at 17 passes or fewer; squared per-qubit remainders, the longest remaining qubit and the count of ops that still
    // need a tile bit all ranked worse than the plain count.
    for (SearchState& c : children) {
      pb.done = c.done;
      pb.remaining = c.remaining;
      pb.first = 0;
      pb.begin_pass();
      claimed.clear();
      const u64 next = pb.first_come(pb.forced_static, &claimed);
      c.rank = 2 * (long)c.remaining - std::min(pb.holds(next, nullptr), PassBuilder::kSaturated);
    }
    // the beam: best rank first (fewest conflicts on ties), one state per done-set
    order.resize(children.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) {
      if (children[a].rank != children[b].rank) return children[a].rank < children[b].rank;
      return children[a].conflicts < children[b].conflicts;
    });
    std::vector<SearchState> kept;
    nodes.emplace_back();
    for (size_t i : order) {
      if ((int)kept.size() >= beam) break;
      bool dup = false;
      for (const SearchState& o : kept) if (o.hash == children[i].hash && o.done == children[i].done) { dup = true; break; }
      if (dup) continue;
      nodes.back().push_back(SearchNode{children[i].parent, children[i].mask});
      kept.push_back(std::move(children[i]));
    }
    for (size_t i = 0; i < kept.size() && finished < 0; ++i) if (kept[i].remaining == 0) finished = (int)i;
    states.swap(kept);
  }
  if (finished < 0) return QSIM_OK;              // nothing shorter than the greedy plan
  std::vector<u64> found(nodes.size());
  for (int d = (int)nodes.size() - 1, at = finished; d >= 0; --d) {
    found[(size_t)d] = nodes[(size_t)d][(size_t)at].mask;
    at = nodes[(size_t)d][(size_t)at].parent;
  }
  // the replay through the hint path must give these passes and no more (it does by construction: same rules, same emit)
  std::vector<u64> replay;
  int replay_passes = 0;
  const std::vector<uint64_t> named(found.begin(), found.end());
  const TileHint hint = {named.data(), (int)named.size()};
  rc = planned_tiles(k, ops_in, &hint, &replay, &replay_passes);
  if (rc) return rc;
  if (replay_passes == (int)found.size() && replay == found) { *masks = found; *n_passes = replay_passes; }
  return QSIM_OK;
}

// ---- many line-qubit triples, one bound ------------------------------------------------------------------------------
// The three qubits on the line bits belong to every tile, so they decide how many passes a plan needs (13 to 15 for the
// rewritten 28-qubit bench list, 13 on 3.5 % of its 3 276 triples).  plan_search_triples searches one op list under many
// triples on host threads: every thread relabels the list for its triple (triple_layout: the rule of
// runner/layout_search.py), runs plan_search with searcher state of its own, and shares one thing with the others, the
// atomic fewest-passes-so-far that bounds every search (SearchBound).  What comes back -- the fewest passes and, for every
// triple that reaches them, its tiles -- is what unbounded searches one by one would give, whatever the thread count.
struct LineTriple { int32_t q[3]; };             // logical qubits that go to index bits 0, 1, 2

// qubit -> index bit with the triple on the line bits: from the identity, the qubit on bit b trades places with t.q[b]
static void triple_layout(int k, const LineTriple& t, int32_t* lay) {
  for (int q = 0; q < k; ++q) lay[q] = q;
  for (int bit = 0; bit < 3; ++bit) {
    int j = 0;
    while (lay[j] != bit) ++j;
    lay[j] = lay[t.q[bit]];
    lay[t.q[bit]] = bit;
  }
}

struct ListSearch {
  int beam = 0, n_threads = 1;
  bool bounded = true, need_bits = false;
  int best = 0;                                  // out: the fewest passes over the lists
  std::vector<int32_t> passes;                   // out, per list: its passes; bounded: -1 where they are more than `best`
  std::vector<std::vector<u64>> masks;           // out, per list: its tiles where it reaches `best` (unbounded: always), else empty
};

// plan_search of n op lists on host threads under one bound: make(t, &ops) writes list t (called on the thread that searches it)
template <class Make>
static int plan_search_lists(int k, size_t n, Make&& make, ListSearch* ts) {
  ts->passes.assign(n, -1);
  ts->masks.assign(n, std::vector<u64>());
  ts->best = 0;
  if (!n) return QSIM_OK;
  (void)tuning();                                // (initialised before the threads start)
  std::atomic<int> best{1 << 30}, bad{0};
  std::atomic<size_t> next{0};
  auto work = [&]() {                            // (everything a search writes is local to it or its own slot of `ts`)
    std::vector<FusedOp> ops;
    std::vector<u64> found;
    for (;;) {
      const size_t t = next.fetch_add(1);
      if (t >= n) return;
      ops.clear();
      make(t, &ops);
      SearchBound bound = {&best, ts->need_bits, false};
      int passes = 0;
      if (plan_search(k, ops, ts->beam, &found, &passes, ts->bounded ? &bound : nullptr)) { bad.store(1); continue; }
      if (bound.cut) continue;
      ts->passes[t] = passes;
      ts->masks[t] = found;
      for (int seen = best.load(); passes < seen && !best.compare_exchange_weak(seen, passes);) {}
    }
  };
  const int nt = (int)std::max<size_t>(1, std::min<size_t>((size_t)std::max(1, ts->n_threads), std::min<size_t>(n, 64)));
  std::vector<std::thread> pool;
  for (int t = 1; t < nt; ++t) pool.emplace_back(work);
  work();
  for (std::thread& t : pool) t.join();
  if (bad.load()) return fail(QSIM_ERR_INVALID, "internal: an op list of a pass search could not be planned");
  ts->best = best.load();
  // a search that ended above the final `best` before `best` fell kept its result: dropped here, like the ones cut
  for (size_t t = 0; t < n && ts->bounded; ++t)
    if (ts->passes[t] != ts->best) {
      ts->masks[t].clear();
      ts->passes[t] = -1;
    }
  return QSIM_OK;
}

// the caller's op list on the index bits of a triple; origin (optional): classified op -> index in the caller's list
static void triple_ops(int k, const LineTriple& t, int n_ops, const int32_t* nq, const int32_t* qubits, const double* mats,
                       std::vector<FusedOp>* ops, std::vector<int32_t>* origin = nullptr) {
  std::vector<int32_t> lay((size_t)k);
  triple_layout(k, t, lay.data());
  for (int i = 0; i < n_ops; ++i) {
    const int32_t q[2] = {lay[qubits[2 * i]], nq[i] == 2 ? lay[qubits[2 * i + 1]] : -1};
    FusedOp o;
    if (!classify_op(nq[i], q, mats + 32 * (size_t)i, &o)) continue;
    ops->push_back(o);
    if (origin) origin->push_back(i);
  }
}

static int plan_search_triples(int k, int n_ops, const int32_t* nq, const int32_t* qubits, const double* mats,
                               const std::vector<LineTriple>& triples, ListSearch* ts) {
  const bool bounded = ts->bounded;
  const int rc = plan_search_lists(k, triples.size(), [&](size_t t, std::vector<FusedOp>* ops) {
    triple_ops(k, triples[t], n_ops, nq, qubits, mats, ops);
  }, ts);
  // (unbounded: the passes of every triple stay, the tiles only of those that reach the fewest)
  for (size_t t = 0; t < triples.size() && !rc && !bounded; ++t) if (ts->passes[t] != ts->best) ts->masks[t].clear();
  return rc;
}

// ---- cyclic plans: the tail of one execution runs with the head of the next ---------------------------------------------
// A list L that is executed again and again is planned as if every execution stood alone, and the last passes of a plan
// carry little (10 and 36 records against 50-60 on the bench list).  Planned across the boundary the ops are the same:
// with L = A.B as a product (A: a head, B: a tail, each in list order) R executions are A (B.A)^(R-1) B, and B.A may need a
// pass fewer than L (12 instead of 13 for the 28-qubit bench list).  Where to cut comes from a plan, not from the list (no
// list suffix of 6 to 320 ops got below 13): L.L is searched, its tiles are replayed through holds / emit / account for the
// pass of every op -- what emit really wrote, not what holds promised -- and the cut is the first pass that holds an op of
// the second copy: A = the first-copy ops of the passes before it, B = the rest.  That is a product of L: the passes are an
// order of L.L in which no op overtakes one it does not commute with, so nothing of B comes before something of A it does
// not commute with.  A, B.A and B are then searched under the same triple; plan_search checks the replay of each.
struct CyclePlan {
  bool found = false;
  int32_t plain = 0;                             // passes of L under the triple
  int32_t passes[3] = {0, 0, 0};                 // head A, steady B.A, tail B
  std::vector<uint8_t> tail;                     // per op of the CALLER's list: 1 = in B (identities: 0)
  std::vector<u64> masks[3];
};

// the pass of every op of `ops` under the named tiles (first come, no placement); false: they do not finish the list
static bool replay_pass_of(int k, const std::vector<FusedOp>& ops, const std::vector<u64>& masks, std::vector<int32_t>* pass_of) {
  pass_of->assign(ops.size(), -1);
  PassBuilder pb(k, ops, k);
  std::vector<size_t> members;
  std::vector<char> emitted;
  std::vector<TileGroup> groups;
  for (size_t p = 0; p < masks.size() && pb.remaining; ++p) {
    pb.begin_pass();
    pb.pass_no = (int)p;
    members.clear();
    pb.holds(masks[p], &members);
    if (members.empty()) return false;
    pb.emit(members, pb.filled(pb.bits_of(masks[p])), &groups, &emitted);
    for (size_t mi = 0; mi < members.size(); ++mi) if (emitted[mi]) (*pass_of)[members[mi]] = (int32_t)p;
    size_t n_emitted = 0;
    pb.account(members, emitted, &n_emitted);
    if (!n_emitted) return false;
  }
  return pb.remaining == 0;
}

// plain_passes (optional, per triple): the passes of L under the triple where the caller knows them; else L is searched too
static int plan_search_cycle(int k, int n_ops, const int32_t* nq, const int32_t* qubits, const double* mats,
                             const std::vector<LineTriple>& triples, const int32_t* plain_passes, int beam, int n_threads,
                             std::vector<CyclePlan>* out) {
  const size_t n = triples.size();
  out->assign(n, CyclePlan());
  std::vector<std::vector<FusedOp>> L(n);
  std::vector<std::vector<int32_t>> origin(n);
  for (size_t t = 0; t < n; ++t) triple_ops(k, triples[t], n_ops, nq, qubits, mats, &L[t], &origin[t]);
  ListSearch ls;
  ls.beam = beam;
  ls.n_threads = n_threads;
  // 1. L.L under every triple, one bound
  int rc = plan_search_lists(k, n, [&](size_t t, std::vector<FusedOp>* ops) {
    *ops = L[t];
    ops->insert(ops->end(), L[t].begin(), L[t].end());
  }, &ls);
  if (rc) return rc;
  // 2. the cut, and B.A under the triples that have one (one bound again: the fewest steady passes)
  std::vector<size_t> cyc;                       // triples with a cut
  std::vector<std::vector<FusedOp>> part[3];     // A, B.A, B per entry of cyc
  std::vector<int32_t> pass_of;
  for (size_t t = 0; t < n; ++t) {
    if (ls.passes[t] < 0) continue;
    std::vector<FusedOp> twice = L[t];
    twice.insert(twice.end(), L[t].begin(), L[t].end());
    const std::vector<FusedOp> planned = planned_ops(twice);
    const size_t m = L[t].size();
    if (planned.size() != twice.size() || !replay_pass_of(k, planned, ls.masks[t], &pass_of)) continue;   // (the probe build's commuting fusion renumbers the ops)
    int32_t cut = 1 << 30;
    for (size_t i = m; i < 2 * m; ++i) cut = std::min(cut, pass_of[i]);
    std::vector<FusedOp> A, B;
    CyclePlan& c = (*out)[t];
    c.tail.assign((size_t)n_ops, 0);
    for (size_t i = 0; i < m; ++i) {
      (pass_of[i] < cut ? A : B).push_back(L[t][i]);
      c.tail[(size_t)origin[t][i]] = pass_of[i] >= cut;
    }
    if (A.empty() || B.empty()) continue;          // no cycle under this triple
    std::vector<FusedOp> BA = B;
    BA.insert(BA.end(), A.begin(), A.end());
    cyc.push_back(t);
    part[0].push_back(A); part[1].push_back(BA); part[2].push_back(B);
  }
  if (cyc.empty()) return QSIM_OK;
  ListSearch steady;
  steady.beam = beam;
  steady.n_threads = n_threads;
  rc = plan_search_lists(k, cyc.size(), [&](size_t j, std::vector<FusedOp>* ops) { *ops = part[1][j]; }, &steady);
  if (rc) return rc;
  std::vector<size_t> kept;                      // entries of cyc at the fewest steady passes
  for (size_t j = 0; j < cyc.size(); ++j) if (steady.passes[j] == steady.best) kept.push_back(j);
  // 3. A and B of those (and L where the caller does not know its passes), each to the end
  ListSearch ends;
  ends.beam = beam;
  ends.n_threads = n_threads;
  ends.bounded = false;
  const size_t per = plain_passes ? 2 : 3;
  rc = plan_search_lists(k, per * kept.size(), [&](size_t j, std::vector<FusedOp>* ops) {
    const size_t which = j % per, at = kept[j / per];
    *ops = which == 0 ? part[0][at] : which == 1 ? part[2][at] : L[cyc[at]];
  }, &ends);
  if (rc) return rc;
  for (size_t i = 0; i < kept.size(); ++i) {
    const size_t t = cyc[kept[i]];
    CyclePlan& c = (*out)[t];
    c.plain = plain_passes ? plain_passes[t] : ends.passes[per * i + 2];
    c.passes[0] = ends.passes[per * i];
    c.passes[1] = steady.passes[kept[i]];
    c.passes[2] = ends.passes[per * i + 1];
    c.masks[0] = ends.masks[per * i];
    c.masks[1] = steady.masks[kept[i]];
    c.masks[2] = ends.masks[per * i + 1];
    // a cycle counts when its steady passes are fewer than the plain plan's and the three tile lists replay through the
    // hint path into exactly the passes counted
    bool ok = c.passes[1] < c.plain;
    for (int w = 0; w < 3 && ok; ++w) {
      std::vector<u64> replay;
      int replay_passes = 0;
      const std::vector<uint64_t> named(c.masks[w].begin(), c.masks[w].end());
      const TileHint hint = {named.data(), (int)named.size()};
      if ((rc = planned_tiles(k, part[w][kept[i]], &hint, &replay, &replay_passes))) return rc;
      ok = replay_passes == c.passes[w] && (int)named.size() == c.passes[w];
    }
    c.found = ok;
  }
  return QSIM_OK;
}

// ---- pass time = max(memory, engine): the placement of the ops that need no tile ----------------------------------------
// The builders above fill every pass first come, and treat its records as free.  They are not: past FIXED_US + its records
// > the memory time of its tile a pass is bound by the gate engine (profiles/r19a_pass_engine_split.txt: 1.45 of 21.3 ms at
// 28 qubits, while the last two passes of the plan carry next to nothing).  Ops that need no tile -- diagonal 1q gates, CZ /
// CR: 43 % of the rewritten bench list -- may run in any pass from the one first come puts them in to the pass of the
// first later op that TARGETS one of their qubits (everything else on their qubits is diagonal there and commutes).  So:
// the named passes are replayed first come and priced (what PassBuilder::emit really writes, by the table); then, pass by
// pass, while the records of a pass cost more than its memory time, the last such op of the pass goes to the pass of its
// window with the most engine slack, if that slack holds it (TileHint::earliest).  Waiting is the builder's own notion, so
// the result is a correct program whatever is moved, and inside its window an op blocks nothing that runs; what could
// still go wrong is the record budget of the receiving pass, hence the replay at the end: a placement that does not give
// the named passes exactly, or that the model does not price lower, is dropped.
// mem_us: per named pass; eng_before / eng_after: modelled engine microseconds per pass; place = false: priced only.
static int plan_balance(int k, const std::vector<FusedOp>& ops_in, const std::vector<u64>& masks, const double* mem_us,
                        const EngineCosts& ec, bool place, std::vector<int32_t>* earliest, std::vector<double>* eng_before,
                        std::vector<double>* eng_after) {
  const std::vector<FusedOp> ops = planned_ops(ops_in);
  const size_t n_pass = masks.size(), n_ops = ops.size();
  earliest->assign(ops_in.size(), 0);
  eng_before->assign(n_pass, 0.0);
  eng_after->assign(n_pass, 0.0);
  if (n_ops != ops_in.size() || !n_pass) return QSIM_OK;              // (the probe build's commuting fusion renumbers the ops)
  std::vector<size_t> members;
  std::vector<char> emitted;
  std::vector<TileGroup> groups;
  std::vector<int32_t> pass_of(n_ops, -1);
  PassBuilder rules(k, ops, k);                                        // (the masks qm / tm of every op)
  // the named passes under a placement: modelled engine time and the pass of every op; false: they do not finish the list
  auto replay = [&](const int32_t* place, std::vector<double>* eng) {
    PassBuilder pb(k, ops, k);
    for (size_t p = 0; p < n_pass && pb.remaining; ++p) {
      pb.begin_pass();
      pb.pass_no = (int)p;
      pb.earliest = place;
      members.clear();
      pb.holds(masks[p], &members);
      if (members.empty()) return false;
      pb.emit(members, pb.filled(pb.bits_of(masks[p])), &groups, &emitted);
      (*eng)[p] = ec.of_pass(groups, k);
      for (size_t mi = 0; mi < members.size(); ++mi) if (emitted[mi]) pass_of[members[mi]] = (int32_t)p;
      size_t n_emitted = 0;
      pb.account(members, emitted, &n_emitted);
      if (!n_emitted) return false;
    }
    return pb.remaining == 0;
  };
  if (!replay(nullptr, eng_before)) return QSIM_OK;
  *eng_after = *eng_before;
  if (!place) return QSIM_OK;                                          // (the caller only wanted the prices)
  const double scale = std::ldexp(1.0, k - (int)ec.v[QSIM_ENGINE_COST_FIT_QUBITS]);
  std::vector<double> slack(n_pass);
  for (size_t p = 0; p < n_pass; ++p) slack[p] = mem_us[p] - (*eng_before)[p];
  // the last pass an op without a tile need may run in: the earliest pass of a later op that targets one of its qubits
  // (not the first such op of the list: CNOTs with a common target commute, and a later one may run a pass earlier)
  std::vector<int32_t> window(n_ops, -1);
  for (size_t i = 0; i < n_ops; ++i) {
    if (ops[i].ntargets) continue;
    window[i] = (int32_t)n_pass - 1;
    for (size_t j = i + 1; j < n_ops; ++j)
      if (rules.tm[j] & rules.qm[i]) window[i] = std::min(window[i], pass_of[j]);
  }
  std::vector<int32_t> placed(n_ops, 0);
  bool any = false;
  for (size_t p = 0; p + 1 < n_pass; ++p)
    for (size_t i = n_ops; i-- > 0 && slack[p] < 0;) {
      if (pass_of[i] != (int32_t)p || window[i] <= (int32_t)p) continue;
      const double us = ec.of_family(priced_family(ops[i])) * scale;
      size_t to = p;
      for (size_t q = p + 1; q <= (size_t)window[i]; ++q) if (to == p || slack[q] > slack[to]) to = q;
      if (slack[to] < us) continue;
      placed[i] = (int32_t)to;
      slack[to] -= us;
      slack[p] += us;
      any = true;
    }
  if (!any) return QSIM_OK;
  // the check: the placement handed back through the hint path gives the named passes, and the model prices them lower
  std::vector<double> check(n_pass, 0.0);
  if (!replay(placed.data(), &check)) return QSIM_OK;
  double before = 0, after = 0;
  for (size_t p = 0; p < n_pass; ++p) { before += std::max(mem_us[p], (*eng_before)[p]); after += std::max(mem_us[p], check[p]); }
  if (!(after < before)) return QSIM_OK;
  *earliest = placed;
  *eng_after = check;
  return QSIM_OK;
}
