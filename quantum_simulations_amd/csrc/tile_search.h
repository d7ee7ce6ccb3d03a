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
static int plan_search(int k, const std::vector<FusedOp>& ops_in, int beam, std::vector<u64>* masks, int* n_passes) {
  beam = std::max(1, std::min(beam > 0 ? beam : kSearchBeamDefault, kSearchBeamMax));
  int rc = planned_tiles(k, ops_in, nullptr, masks, n_passes);
  if (rc) return rc;
  const int greedy_passes = *n_passes;
  const std::vector<FusedOp> ops = planned_ops(ops_in);
  PassBuilder pb(k, ops, k);
  if (greedy_passes <= 1 || k - pb.low <= pb.cap) return QSIM_OK;      // (one tile holds every qubit: nothing to choose)
  const size_t n_ops = pb.n_ops;

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
    children.clear();
    for (size_t si = 0; si < states.size(); ++si) {
      const SearchState& s = states[si];
      pb.done = s.done;
      pb.remaining = s.remaining;
      pb.first = 0;
      pb.begin_pass();
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
