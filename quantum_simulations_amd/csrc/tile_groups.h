// tile_groups.h -- register-group emission: the ops of one pass -> register groups of <= kGroupBits tile bits and their
// records.  Part of the single translation unit qsim_hip.hip (included there, in order; not a standalone header).
// Host only: nothing here touches the device.

// fn(own) for every three set bits of `mask` (own: the three bits as a mask), lowest bits first
template <class Fn>
static void for_each_triple(unsigned mask, Fn&& fn) {
  for (unsigned a = mask; a; a &= a - 1)
    for (unsigned b = a & (a - 1); b; b &= b - 1)
      for (unsigned c = b & (b - 1); c; c &= c - 1) fn((a & -a) | (b & -b) | (c & -c));
}

// Phase gates with ONE register bit and the same predicate (lane bits + outer bits) are merged
// (the QFT's CR(k, a), CR(k, b), CR(k, c) for the group's register bits a, b, c): diagonal
// gates commute with everything except a non-diagonal gate on one of their bits, so an open
// accumulator is written out before such a gate on a register bit it has touched, or at the
// end of the group.  One record instead of up to three: the gate loop is instruction-issue bound.
struct PhaseRuns {
  struct Acc { uint16_t blk; u64 outer; double2 phi[3]; unsigned touched; };
  std::vector<Acc> open;

  static int run_bytes(unsigned touched) { const int n = __builtin_popcount(touched); return desc_bytes(n == 1 ? 2 : (n == 2 ? 6 : 14)); }
  int reserve() const {               // what the open runs may need of the record budget
    int bytes = 0;
    for (const Acc& acc : open) bytes += run_bytes(acc.touched);
    return bytes;
  }
  // one more phase on register bit r under the predicate (blk, outer)
  void add(uint16_t blk, u64 outer, int r, double2 phase) {
    size_t i = 0;
    while (i < open.size() && !(open[i].blk == blk && open[i].outer == outer)) ++i;
    if (i == open.size()) {
      Acc acc;
      acc.blk = blk; acc.outer = outer; acc.touched = 0;
      for (int e = 0; e < 3; ++e) acc.phi[e] = make_double2(1.0, 0.0);
      open.push_back(acc);
    }
    Acc& acc = open[i];
    acc.phi[r] = cmul(acc.phi[r], phase);
    acc.touched |= 1u << r;
  }
  // one phase on one register bit, under the predicate of `pred`
  static TileDesc single(const TileDesc& pred, int r, double2 v) {
    TileDesc s1 = pred;
    const int fam = phase_family(v);
    s1.opcode = (uint8_t)(fam + (1u << r));
    if (fam == OPC_PHASE) { s1.m[0] = v.x; s1.m[1] = v.y; s1.nd = 2; }
    return s1;
  }
  static int cost1(double2 v) {   // vector instructions of the single form (4 registers)
    if (!tuning().tile_special) return 16;
    return (v.x == -1 && v.y == 0) ? 8 : ((v.x == 0 && (v.y == 1 || v.y == -1)) ? 12 : 16);
  }
  // write run i out behind `gates`; returns the bytes of its records
  int flush(size_t i, std::vector<TileDesc>* gates) {
    const Acc acc = open[i];
    open.erase(open.begin() + (long)i);
    const size_t from = gates->size();
    TileDesc d;
    std::memset(&d, 0, sizeof d);
    d.blk_mask = acc.blk;
    d.outer_mask = acc.outer;
    double2 m[3];
    int nm = 0, regs[3];
    for (int r = 0; r < 3; ++r) if (acc.touched & (1u << r)) { regs[nm] = r; m[nm++] = acc.phi[r]; }
    auto put = [&](int at, double2 v) { d.m[2 * at] = v.x; d.m[2 * at + 1] = v.y; };
    // merged run: 6 (two bits) or 7 (three bits) registers x 4 instructions, one record instead of nm
    int separate = 0;
    for (int e = 0; e < nm; ++e) separate += cost1(m[e]);
    if (nm == 1 || separate < (nm == 2 ? 24 : 28)) {
      for (int e = 0; e < nm; ++e) gates->push_back(single(d, regs[e], m[e]));
    } else if (nm == 2) {
      d.opcode = (uint8_t)(OPC_DIAGR + (acc.touched == 3 ? 0 : acc.touched == 5 ? 1 : 2));
      put(0, m[0]); put(1, m[1]); put(2, cmul(m[0], m[1])); d.nd = 6;
      gates->push_back(d);
    } else {                          // a, b, c | ab, ac, bc, abc
      d.opcode = (uint8_t)(OPC_DIAGR + 3);
      const double2 ab = cmul(m[0], m[1]);
      put(0, m[0]); put(1, m[1]); put(2, m[2]);
      put(3, ab); put(4, cmul(m[0], m[2])); put(5, cmul(m[1], m[2])); put(6, cmul(ab, m[2]));
      d.nd = 14;
      gates->push_back(d);
    }
    int bytes = 0;
    for (size_t g = from; g < gates->size(); ++g) bytes += desc_bytes((*gates)[g]);
    return bytes;
  }
};

// Split one pass's ops (list order) into register groups of <= kGroupBits target tile bits and
// collect their descriptors.  Ops that do not fit the record budget stay un-emitted (they and
// everything that depends on them wait for the next launch).
struct GroupEmitter {
  // The FIRST group of a full tile is free of its LDS read when it lies above the line bits (the kernel loads the
  // tile in that layout, OPC_GROUP_DIRECT): such a triple wins unless another one holds kDirectWorth more ops.
  // (the preference off / stronger: see the variants counted in PassBuilder::emit)
  static constexpr int kDirectWorth = 2;

  const std::vector<FusedOp>& ops;
  const std::vector<size_t>& members;
  const std::vector<int>& high;
  const int T, low = kTileLow;
  std::vector<TileGroup>* out;
  std::vector<char>* emitted;
  const unsigned line_bits = (1u << kTileLow) - 1;
  const bool merge_on = tuning().tile_merge_diag != 0;
  const bool direct_ends;             // (serialize_pass: full tiles only)
  double pass_scale = 1.0;            // product of the factors of the pass's unscaled Hadamard butterflies (OPC_HAD1)
  std::vector<char> done;
  size_t left;
  int used = 0;                       // bytes of the records written so far
  int regs[kGroupBits] = {0, 0, 0};   // the tile bits of the group being written, ascending
  // the group set aside for the end (reserve_last)
  std::vector<char> reserved;
  unsigned last_own = 0;
  int reserve_bytes = 0;
  size_t n_reserved = 0;

  struct Item { FusedOp op; size_t mi; int with_next; };   // with_next: record bytes of the second half of a pair (both or neither fit)
  struct Half { FusedOp op; size_t stands_for; };          // the control = 1 record of a pair, and which op of the group it stands for

  GroupEmitter(const std::vector<FusedOp>& ops_, const std::vector<size_t>& members_, const std::vector<int>& high_, int T_,
               std::vector<TileGroup>* out_, std::vector<char>* emitted_)
      : ops(ops_), members(members_), high(high_), T(T_), out(out_), emitted(emitted_),
        direct_ends(tuning().tile_direct && T_ == kTileBitsMax), done(members_.size(), 0), left(members_.size()),
        reserved(members_.size(), 0) {}

  // emitted[mi] = 1 for every member that got its records; last_search: the last group is chosen first, from the end
  static void emit(const std::vector<FusedOp>& ops, const std::vector<size_t>& members, const std::vector<int>& high, int T,
                   std::vector<TileGroup>* out, std::vector<char>* emitted, bool last_search = false) {
    GroupEmitter e(ops, members, high, T, out, emitted);
    out->clear();
    if (e.direct_ends && last_search && members.size() > 1) e.reserve_last();
    while (e.left > e.n_reserved) {
      std::vector<size_t> grp;          // indices into members
      unsigned claimed = 0;
      e.next_group(&grp, &claimed);
      if (grp.empty()) break;           // record budget exhausted: the rest waits for the next launch
      if (e.write_group(grp, claimed)) break;   // record budget exhausted inside the group
    }
    if (e.n_reserved) e.write_reserved();
    e.move_last_forward();
    e.apply_scale();
  }

  int tile_pos(int b) const {
    if (b < low) return b;
    for (size_t j = 0; j < high.size(); ++j) if (high[j] == b) return low + (int)j;
    return -1;
  }
  int reg_pos(int tile_bit) const {
    for (int j = 0; j < kGroupBits; ++j) if (regs[j] == tile_bit) return j;
    return -1;
  }
  // a member as the two searches see it: its qubits, the tile positions of its targets, an estimate of its record bytes
  struct Pending { size_t mi; u64 qm; unsigned need; int bytes; };
  Pending pending(size_t mi, int phase_bytes) const {
    const FusedOp& o = ops[members[mi]];
    const OpShape shape = op_shape(o);
    unsigned need = 0;
    for (int t = 0; t < o.ntargets; ++t) need |= 1u << tile_pos(o.target[t]);
    return Pending{mi, op_qmask(o), need, phase_bytes ? phase_bytes : desc_bytes(shape.nd)};
  }

  // ops a last group owning the tile bits `own` would hold: the TERMINAL ops (ops that no op outside the set follows on
  // any of their qubits), from the end of the list, within half the record budget
  int terminal(const std::vector<Pending>& tail, unsigned own, std::vector<char>* mark) {
    u64 blocked = 0;
    int count = 0, bytes = kGroupRecordBytes;
    for (size_t mi = members.size(); mi-- > 0;) {
      const Pending& t = tail[mi];
      if ((blocked & t.qm) || (t.need & ~own) || bytes + t.bytes > kTileRecordBudget / 2) { blocked |= t.qm; continue; }
      bytes += t.bytes;
      ++count;
      if (mark) (*mark)[mi] = 1;
    }
    if (mark) reserve_bytes = bytes;
    return count;
  }
  // The LAST group of a full tile is free of its LDS write-back when it lies above the line bits (the kernel stores
  // the tile in that layout, OPC_END_DIRECT).  Chosen first, from the END of the list: the triple of bits above the
  // line bits that holds the most TERMINAL ops; those ops are set aside, the groups in front of them are built as
  // before, and they are written last.
  void reserve_last() {
    std::vector<Pending> tail;
    unsigned cand = 0;
    for (size_t mi = 0; mi < members.size(); ++mi) {
      tail.push_back(pending(mi, ops[members[mi]].kind == TG_PHASE ? 48 : 0));
      cand |= tail[mi].need & ~line_bits;
    }
    int best = 0;
    while (__builtin_popcount(cand) < kGroupBits)          // fewer than three target bits above the line bits: pad
      for (int b = T - 1; b >= low; --b) if (!(cand & (1u << b))) { cand |= 1u << b; break; }
    for_each_triple(cand, [&](unsigned own) {
      const int count = terminal(tail, own, nullptr);
      if (count > best) { best = count; last_own = own; }
    });
    if (best > 0 && (size_t)best < members.size()) {
      n_reserved = (size_t)terminal(tail, last_own, &reserved);
      used = reserve_bytes;
    } else {
      last_own = 0;
    }
  }
  // the group set aside for the end: an op of it waits for the next launch with everything un-emitted that it follows
  void write_reserved() {
    used -= reserve_bytes;
    std::vector<size_t> grp;
    u64 blocked = 0;
    for (size_t mi = 0; mi < members.size(); ++mi) {
      if (done[mi]) continue;
      const u64 qm = op_qmask(ops[members[mi]]);
      if (!reserved[mi] || (blocked & qm)) { blocked |= qm; continue; }
      grp.push_back(mi);
    }
    if (!grp.empty()) write_group(grp, last_own);
  }

  // ops a group owning the tile bits `own` (mask) would hold, in list order, within the record budget;
  // own == 0: first come (bits are claimed as ops need them)
  int select(const std::vector<Pending>& pend, unsigned own, std::vector<size_t>* grp_out, unsigned* claimed_out) const {
    const bool first_come = own == 0;
    u64 blocked = 0;
    int est = used + kGroupRecordBytes, count = 0;
    unsigned claimed = own;
    for (const Pending& pd : pend) {
      bool ok = !(blocked & pd.qm);
      if (ok && first_come && __builtin_popcount(claimed | pd.need) > kGroupBits) ok = false;
      if (ok && !first_come && (pd.need & ~own)) ok = false;
      if (ok && est + pd.bytes > kTileRecordBudget) ok = false;
      if (!ok) { blocked |= pd.qm; continue; }
      claimed |= pd.need;
      est += pd.bytes;
      ++count;
      if (grp_out) grp_out->push_back(pd.mi);
    }
    if (claimed_out) *claimed_out = first_come ? claimed : own;
    return count;
  }
  // a group of `count` ops on the tile bits `own_bits`; a first group of a full tile prefers a triple above the line bits
  int score(int count, unsigned own_bits) const {
    const bool want_direct = out->empty() && direct_ends;
    return count * 2 + ((want_direct && !(own_bits & line_bits)) ? 2 * kDirectWorth - 1 : 0);
  }
  // Which three tile bits does the group own?  First come (an op that still fits claims the bits it needs)
  // was the only rule up to r02a; now every triple of the pending ops' target bits is also tried and the one
  // that lets the group hold the most ops wins (ties: first come).  A group change is an LDS round trip of the
  // tile plus a barrier (~4 % of a tile's time each): 102 -> 86 groups on the 18 passes of the bench circuit.
  // Estimate of the record budget: a phase gate that may be merged with others (OPC_DIAGR) is counted as a
  // bare header; the exact budget is enforced when the group is written out (a group that overflows is cut
  // there, the rest waits for the next pass).
  void next_group(std::vector<size_t>* grp, unsigned* claimed) const {
    std::vector<Pending> pend;
    pend.reserve(left);
    unsigned cand_mask = 0;           // tile positions that pending ops target
    for (size_t mi = 0; mi < members.size(); ++mi) {
      if (done[mi] || reserved[mi]) continue;
      pend.push_back(pending(mi, (merge_on && op_shape(ops[members[mi]]).family == OPC_PHASE) ? 16 : 0));
      cand_mask |= pend.back().need;
    }
    unsigned best_own = 0;
    unsigned fc_claimed = 0;
    const int fc_count = select(pend, 0, nullptr, &fc_claimed);
    int best_score = score(fc_count, fc_claimed);
    if (tuning().tile_group_search && __builtin_popcount(cand_mask) > kGroupBits)
      for_each_triple(cand_mask, [&](unsigned own) {
        const int count = select(pend, own, nullptr, nullptr);
        if (count > 0 && score(count, own) > best_score) { best_score = score(count, own); best_own = own; }
      });
    select(pend, best_own, grp, claimed);
  }

  // The group's ops in emission order.  Peephole (tuning().tile_mux): a controlled gate C(V) whose control lies
  // OUTSIDE the tile (a per-tile predicate) next to an unconditional 1q gate U on its target -- nothing between
  // them touching the target -- becomes two predicated records at U's place: control = 1 -> U V (or V U when U comes
  // first), control = 0 -> U.  A tile runs exactly one of the two, so the pair costs one 2x2 instead of 2x2 + V; for
  // V = X (CNOT, 3 of 4 cases on the bench circuit) that removes 16 half-rate v_swap_b32 per thread.
  std::vector<Item> mux_pairs(const std::vector<size_t>& grp) const {
    const size_t ng = grp.size();
    std::vector<Item> seq;
    seq.reserve(ng + 4);
    std::vector<char> gone(ng, 0), paired(ng, 0);
    std::vector<Half> first_half(ng);        // for a paired U: the control = 1 record emitted in front of it
    auto op_at = [&](size_t g) -> const FusedOp& { return ops[members[grp[g]]]; };
    auto is_plain_1q = [](const FusedOp& u) { return (u.kind == TG_DENSE1 || u.kind == TG_ANTI1) && u.control < 0; };
    for (size_t p = 0; p < (tuning().tile_mux ? ng : 0); ++p) {
      const FusedOp& cv = op_at(p);
      if (gone[p] || paired[p] || cv.control < 0 || tile_pos(cv.control) >= 0) continue;
      if (cv.kind != TG_SWAP1 && cv.kind != TG_ANTI1 && cv.kind != TG_DENSE1) continue;
      const u64 tbit = 1ull << cv.target[0];
      long partner = -1;
      bool u_first = false;
      for (size_t q = p + 1; q < ng; ++q) {              // U after C(V)
        if (gone[q] || !(op_qmask(op_at(q)) & tbit)) continue;
        if (is_plain_1q(op_at(q)) && !paired[q]) partner = (long)q;
        break;
      }
      if (partner < 0) {                                 // U in front of C(V) -- unless C(V) can sink into the write-back
        bool touched_later = false;
        for (size_t q = p + 1; q < ng && !touched_later; ++q) touched_later = !gone[q] && (op_qmask(op_at(q)) & tbit);
        if (cv.kind == TG_SWAP1 && tuning().tile_sink_swaps && !touched_later) continue;
        for (size_t q = p; q-- > 0;) {
          if (gone[q] || !(op_qmask(op_at(q)) & tbit)) continue;
          if (is_plain_1q(op_at(q)) && !paired[q]) { partner = (long)q; u_first = true; }
          break;
        }
      }
      if (partner < 0) continue;
      const FusedOp& u = op_at((size_t)partner);
      Half& half = first_half[(size_t)partner];
      half.op = cv;                                      // control = 1 half: keeps C(V)'s control and bookkeeping
      if (u_first) mul2x2(cv.m, u.m, half.op.m); else mul2x2(u.m, cv.m, half.op.m);
      set_1q_kind(&half.op);
      half.stands_for = p;
      paired[(size_t)partner] = 1;
      gone[p] = 1;
    }
    for (size_t q = 0; q < ng; ++q) {
      if (gone[q]) continue;
      const FusedOp& u = op_at(q);
      if (!paired[q]) { seq.push_back(Item{u, grp[q], 0}); continue; }
      const FusedOp& a = first_half[q].op;
      FusedOp b = u;                                       // control = 0 half: U under the complementary predicate
      b.control = a.control;
      b.control_zero = true;
      b.nq = 2;
      b.qubits[1] = a.control;
      seq.push_back(Item{a, grp[first_half[q].stands_for], desc_bytes(op_shape(b).nd)});
      seq.push_back(Item{b, grp[q], 0});
    }
    return seq;
  }

  // The record of one op on the registers of the group (for a phase gate that joins a run: its predicate and, in `reg_mask`,
  // its register bit); touched_later: the qubits that the ops behind it in the group touch.
  TileDesc describe(const FusedOp& o, const OpShape& shape, u64 touched_later, unsigned* reg_mask) {
    TileDesc d;
    std::memset(&d, 0, sizeof d);
    int ctrl_reg = -1;
    *reg_mask = 0;
    auto require_one = [&](int qubit) {      // a control / phase bit
      const int p = tile_pos(qubit);
      if (p < 0) { d.outer_mask |= 1ull << qubit; return; }
      const int r = reg_pos(p);
      if (r >= 0) { *reg_mask |= 1u << r; ctrl_reg = r; }
      else d.blk_mask |= (uint16_t)(1u << p);
    };
    auto put = [&](int at, double2 v) { d.m[2 * at] = v.x; d.m[2 * at + 1] = v.y; };
    if (o.kind == TG_PHASE) {
      for (int t = 0; t < o.nbits; ++t) require_one(o.bits[t]);
      d.opcode = (uint8_t)(shape.family + *reg_mask);
      if (shape.nd) { put(0, o.m[0]); d.nd = 2; }
    } else if (o.kind == TG_DENSE2) {
      d.opcode = (uint8_t)(OPC_DENSE2 + 3 * reg_pos(tile_pos(o.target[0])) + reg_pos(tile_pos(o.target[1])));
      for (int e = 0; e < 16; ++e) put(e, o.m[e]);
      d.nd = 32;
    } else {
      const int J = reg_pos(tile_pos(o.target[0]));
      if (o.control >= 0 && o.control_zero) { d.outer_mask |= 1ull << o.control; d.outer_zero = true; }   // (outside the tile by construction)
      else if (o.control >= 0) require_one(o.control);
      d.opcode = (uint8_t)(shape.family + opc_1q_variant(J, ctrl_reg));
      // X / CNOT that nothing later touches are sunk into the write-back: OPC_ASWAP1
      if (shape.family == OPC_SWAP1 && tuning().tile_sink_swaps &&
          !(touched_later & (1ull << o.target[0])) && !(ctrl_reg >= 0 && (touched_later & (1ull << o.control))))
        d.opcode = (uint8_t)(OPC_ASWAP1 + opc_1q_variant(J, ctrl_reg));
      if (shape.family == OPC_HAD1) {
        pass_scale *= o.m[0].x;
      } else if (shape.family == OPC_REAL1) {
        d.m[0] = o.m[0].x; d.m[1] = o.m[1].x; d.m[2] = o.m[2].x; d.m[3] = o.m[3].x; d.nd = 4;
      } else if (shape.family == OPC_ANTI1) {
        put(0, o.m[1]); put(1, o.m[2]); d.nd = 4;
      } else if (shape.family == OPC_DENSE1) {
        for (int e = 0; e < 4; ++e) put(e, o.m[e]);
        d.nd = 8;
      }
    }
    return d;
  }

  // Write one register group: the ops `grp` (indices into members, list order) on the tile bits `claimed`.
  // Returns true when the record budget ended inside the group.
  bool write_group(const std::vector<size_t>& grp, unsigned claimed) {
    std::vector<int> S;               // tile bits of this group
    for (unsigned m = claimed; m; m &= m - 1) S.push_back(__builtin_ctz(m));
    // pad the group with the highest unused tile bits (high bits keep LDS accesses contiguous)
    for (int b = T - 1; (int)S.size() < kGroupBits && b >= 0; --b)
      if (std::find(S.begin(), S.end(), b) == S.end()) S.push_back(b);
    std::sort(S.begin(), S.end());
    TileGroup tg;
    for (int j = 0; j < 3; ++j) tg.s[j] = regs[j] = S[j];
    tg.qmask = 0;
    used += kGroupRecordBytes;
    PhaseRuns runs;
    const std::vector<Item> seq = mux_pairs(grp);
    // qubits touched by the ops AFTER position i of the group
    std::vector<u64> later(seq.size() + 1, 0);
    for (size_t i = seq.size(); i-- > 0;) later[i] = later[i + 1] | op_qmask(seq[i].op);
    bool cut = false;
    size_t gi = 0;
    for (const Item& item : seq) {
      const u64 touched_later = later[++gi];
      const FusedOp& o = item.op;
      const OpShape shape = op_shape(o);
      {   // exact budget: records written so far + what the open runs may need + this op (a mergeable
          // phase may grow a run to its largest form)
        const bool mergeable = merge_on && o.kind == TG_PHASE;
        if (used + runs.reserve() + (mergeable ? desc_bytes(14) : desc_bytes(shape.nd)) + item.with_next > kTileRecordBudget) { cut = true; break; }
      }
      done[item.mi] = 1;
      (*emitted)[item.mi] = 1;
      --left;
      tg.qmask |= op_qmask(o);
      unsigned reg_mask = 0;
      const TileDesc d = describe(o, shape, touched_later, &reg_mask);
      if (o.kind == TG_PHASE && merge_on && __builtin_popcount(reg_mask) == 1) {   // (every phase family: -1 / +-i join the runs too)
        runs.add(d.blk_mask, d.outer_mask, __builtin_ctz(reg_mask), o.m[0]);
        continue;
      }
      if (o.kind != TG_PHASE) {               // a non-diagonal gate: its targets end the open phase runs on them
        unsigned tmask = 0;
        for (int t = 0; t < o.ntargets; ++t) tmask |= 1u << reg_pos(tile_pos(o.target[t]));
        for (size_t i = runs.open.size(); i-- > 0;) if (runs.open[i].touched & tmask) used += runs.flush(i, &tg.gates);
      }
      used += desc_bytes(d);
      tg.gates.push_back(d);
    }
    while (!runs.open.empty()) used += runs.flush(0, &tg.gates);
    if (!tg.gates.empty()) out->push_back(tg);
    else used -= kGroupRecordBytes;
    return cut;
  }

  // The LAST group of a full tile is free of its LDS write-back when it lies above the line bits (OPC_END_DIRECT):
  // a last group that does not is moved in front of its predecessors as long as it shares no qubit with them
  // (groups on disjoint qubits commute), while that leaves a direct-capable group at the end.
  void move_last_forward() {
    if (!(tuning().tile_direct && T == kTileBitsMax && out->size() > 1 && out->back().s[0] < low)) return;
    size_t at = out->size() - 1;
    while (at > 0 && !((*out)[at].qmask & (*out)[at - 1].qmask)) { std::swap((*out)[at], (*out)[at - 1]); --at; }
    if (out->back().s[0] < low)       // nothing gained: keep the original order
      while (at + 1 < out->size()) { std::swap((*out)[at], (*out)[at + 1]); ++at; }
  }
  // a global factor commutes with everything: applied once
  void apply_scale() {
    if (!(pass_scale != 1.0 && !out->empty())) return;
    // ... for free when the pass has an unconditional dense / real / anti-diagonal 1q gate (every amplitude goes
    // through its matrix: scale the matrix); else as one OPC_SCALE record at the end
    TileDesc* host = nullptr;
    for (TileGroup& g : *out)
      for (TileDesc& d : g.gates) {
        if (factor_host_doubles(d.opcode) && !d.blk_mask && !d.outer_mask && !host) host = &d;
      }
    if (host) {
      for (int e = 0; e < host->nd; ++e) host->m[e] *= pass_scale;
    } else {
      TileDesc d;
      std::memset(&d, 0, sizeof d);
      d.opcode = OPC_SCALE;
      d.m[0] = pass_scale;
      d.nd = 1;
      out->back().gates.push_back(d);
    }
  }
};

// ---- OPC_REAL1 -> OPC_UNIT1 on the way to the device ------------------------------------------------------------------
// A planned pass image keeps its real 2x2 records as OPC_REAL1 (a multiply and an FMA per output component).  Before
// run_fused launches (and caches) an image, every UNCONDITIONAL one -- case in header dword 0, so no predicate; variant
// 0..2, so no register control: every amplitude goes through its matrix -- that unit_real_of accepts is rewritten in
// place into OPC_UNIT1: same record size, doubles p, q | s, 0.  The product of the factors s goes where the Hadamard
// factors of the pass went (GroupEmitter::apply_scale): into the matrix of an unconditional dense / real / anti-diagonal
// record.  A pass without another such record keeps its LAST qualifying record as OPC_REAL1 and folds the factor into it:
// an OPC_SCALE record is priced as a phase record, and OPC_UNIT1 + OPC_SCALE above OPC_REAL1.  (A pass that has an
// OPC_SCALE record has no unconditional real 2x2 -- apply_scale would have used it -- so there is nothing to rewrite.)
// Returns the number of records rewritten.
static int lower_unit_real(TileArgs* a) {
  if (!tuning().tile_unit || !tuning().tile_special) return 0;
  unsigned char* const base = reinterpret_cast<unsigned char*>(a);
  auto get32 = [&](int at) { uint32_t v; std::memcpy(&v, base + at, 4); return v; };
  auto put32 = [&](int at, uint32_t v) { std::memcpy(base + at, &v, 4); };
  std::vector<int> unit;              // offsets of the records to rewrite
  int host = -1, host_next = 0;
  for (int off = kTileStreamOff;;) {
    // (an unconditional record carries its case in header dword 0; a predicated one OPC_PRED_*)
    const int entry = (int)(get32(off) / 4), next = (int)get32(off + 4);
    if (entry == OPC_END || entry == OPC_END_DIRECT) break;
    if (next <= off || next + kEndRecordBytes > kTileArgBytes) return 0;     // (not a stream serialize_pass wrote)
    if (factor_host_doubles(entry)) {
      double m[4];
      for (int e = 0; e < 4; ++e) std::memcpy(&m[e], base + record_double_at(off, next, 4, e), 8);
      if (entry >= OPC_REAL1 && entry < OPC_REAL1 + 3 && unit_real_of(m)) unit.push_back(off);
      else if (host < 0) { host = off; host_next = next; }
    }
    off = next;
  }
  if (host < 0) {
    if (unit.size() < 2) return 0;
    host = unit.back();
    host_next = (int)get32(host + 4);
    unit.pop_back();
  }
  double factor = 1.0;
  for (int off : unit) {
    double m[4];
    const int next = (int)get32(off + 4);
    for (int e = 0; e < 4; ++e) std::memcpy(&m[e], base + record_double_at(off, next, 4, e), 8);
    UnitReal u;
    unit_real_of(m, &u);
    factor *= u.s;
    const uint32_t J = get32(off) / 4 - OPC_REAL1;
    const uint32_t entry = OPC_UNIT1 + 4 * J + 2 * (u.form_a ? 1u : 0u) + (u.neg ? 1u : 0u);
    put32(off, 4 * entry);
    put32(off + 12, (4 * entry) << 16);
    const double out[4] = {u.p, u.q, u.s, 0.0};
    for (int e = 0; e < 4; ++e) std::memcpy(base + record_double_at(off, next, 4, e), &out[e], 8);
  }
  if (unit.empty()) return 0;
  const int host_nd = factor_host_doubles((int)(get32(host) / 4));
  for (int e = 0; e < host_nd; ++e) {
    double v;
    unsigned char* at = base + record_double_at(host, host_next, host_nd, e);
    std::memcpy(&v, at, 8);
    v *= factor;
    std::memcpy(at, &v, 8);
  }
  return (int)unit.size();
}
