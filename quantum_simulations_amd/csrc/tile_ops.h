// tile_ops.h -- the op model of the fused-pass planner: what an op is, what its record costs, and the op-list rewrites.
// Part of the single translation unit qsim_hip.hip (included there, in order; not a standalone header).
// Host only: nothing here touches the device.
enum { TG_DENSE1 = 0, TG_PHASE = 1, TG_DENSE2 = 2, TG_ANTI1 = 3, TG_SWAP1 = 4 };   // FusedOp::kind

struct FusedOp {
  int kind;            // TG_DENSE1 / TG_ANTI1 / TG_SWAP1 (target, optional control), TG_PHASE, TG_DENSE2
  int target[2];       // 1q kinds: target[0]; TG_DENSE2: (qa, qb)
  int ntargets;
  int control;         // 1q kinds: control qubit or -1
  int bits[2];         // TG_PHASE: qubits that must be 1
  int nbits;
  int qubits[2];       // every qubit the op touches (for ordering)
  int nq;
  double2 m[16];
  int nm;              // matrix entries (4, 1 or 16)
  int halvings;        // algorithmic bytes = 32 B x 2^(k - halvings)  
  double absorbed;     // algorithmic bytes of the gates fused into this one, as a fraction of 32 B x 2^k
  bool control_zero;   // the control must be 0 instead of 1 (only produced by GroupEmitter::mux_pairs, for a control outside the tile)
};

static void set_1q_kind(FusedOp* o) {   // o->m holds the 2x2
  const bool zero_diag = o->m[0].x == 0 && o->m[0].y == 0 && o->m[3].x == 0 && o->m[3].y == 0;
  const bool ones = o->m[1].x == 1 && o->m[1].y == 0 && o->m[2].x == 1 && o->m[2].y == 0;
  o->kind = zero_diag ? (ones ? TG_SWAP1 : TG_ANTI1) : TG_DENSE1;
}

// Same classification as gate_1q / gate_2q; returns false for an identity.
static bool classify_op(int nq, const int32_t* q, const double* U, FusedOp* o) {
  o->nq = nq;
  o->qubits[0] = q[0];
  o->qubits[1] = nq == 2 ? q[1] : -1;
  o->control = -1;
  o->nbits = 0;
  o->ntargets = 0;
  o->halvings = 0;
  o->absorbed = 0.0;
  o->control_zero = false;
  auto C = [&](int i) { return make_double2(U[2 * i], U[2 * i + 1]); };
  if (nq == 1) {
    const bool diag = is_zero(U[2], U[3]) && is_zero(U[4], U[5]);
    if (diag && is_one(U[0], U[1])) {
      if (is_one(U[6], U[7])) return false;
      o->kind = TG_PHASE; o->bits[0] = q[0]; o->nbits = 1; o->m[0] = C(3); o->nm = 1;
      return true;
    }
    o->target[0] = q[0]; o->ntargets = 1;
    for (int i = 0; i < 4; ++i) o->m[i] = C(i);
    o->nm = 4;
    set_1q_kind(o);
    return true;
  }
  auto z = [&](int r, int c) { return is_zero(U[2 * (4 * r + c)], U[2 * (4 * r + c) + 1]); };
  auto one = [&](int r, int c) { return is_one(U[2 * (4 * r + c)], U[2 * (4 * r + c) + 1]); };
  bool offdiag_zero = true;
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c)
      if (r != c && !z(r, c)) offdiag_zero = false;
  const bool ctrl_a = one(0, 0) && one(1, 1) && z(0, 1) && z(1, 0) && z(0, 2) && z(0, 3) && z(1, 2) &&
                      z(1, 3) && z(2, 0) && z(2, 1) && z(3, 0) && z(3, 1);
  const bool ctrl_b = one(0, 0) && one(2, 2) && z(0, 2) && z(2, 0) && z(0, 1) && z(0, 3) && z(2, 1) &&
                      z(2, 3) && z(1, 0) && z(1, 2) && z(3, 0) && z(3, 2);
  if (offdiag_zero && one(0, 0) && one(1, 1) && one(2, 2)) {
    if (one(3, 3)) return false;
    o->kind = TG_PHASE; o->bits[0] = q[0]; o->bits[1] = q[1]; o->nbits = 2; o->m[0] = C(15); o->nm = 1;
    return true;
  }
  if (ctrl_a || ctrl_b) {
    o->control = ctrl_a ? q[0] : q[1];
    o->target[0] = ctrl_a ? q[1] : q[0];
    o->ntargets = 1;
    if (ctrl_a) { o->m[0] = C(10); o->m[1] = C(11); o->m[2] = C(14); o->m[3] = C(15); }
    else        { o->m[0] = C(5);  o->m[1] = C(7);  o->m[2] = C(13); o->m[3] = C(15); }
    o->nm = 4;
    set_1q_kind(o);
    if (o->kind == TG_DENSE1 && o->m[1].x == 0 && o->m[1].y == 0 && o->m[2].x == 0 && o->m[2].y == 0 &&
        o->m[0].x == 1 && o->m[0].y == 0) {   // controlled phase written as CU: diag(1, d)
      o->kind = TG_PHASE; o->bits[0] = q[0]; o->bits[1] = q[1]; o->nbits = 2; o->m[0] = o->m[3]; o->nm = 1;
      o->ntargets = 0; o->control = -1;
    }
    return true;
  }
  o->kind = TG_DENSE2; o->target[0] = q[0]; o->target[1] = q[1]; o->ntargets = 2;
  for (int i = 0; i < 16; ++i) o->m[i] = C(i);
  o->nm = 16;
  const bool swap = one(0, 0) && one(3, 3) && one(1, 2) && one(2, 1) && z(1, 1) && z(2, 2) && z(0, 1) && z(0, 2) &&
                    z(0, 3) && z(1, 0) && z(1, 3) && z(2, 0) && z(2, 3) && z(3, 0) && z(3, 1) && z(3, 2);
  o->halvings = swap ? 1 : 0;   // SWAP only exchanges |01> and |10>
  return true;
}

static inline u64 op_qmask(const FusedOp& o) {
  u64 m = 1ull << o.qubits[0];
  if (o.nq == 2) m |= 1ull << o.qubits[1];
  return m;
}

static inline double2 cmul(double2 a, double2 b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
static inline double2 cadd(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
static inline void mul2x2(const double2* a, const double2* b, double2* out) {   // out = a b (2x2, row major; out aliases neither)
  for (int r = 0; r < 2; ++r)
    for (int c = 0; c < 2; ++c) out[2 * r + c] = cadd(cmul(a[2 * r], b[c]), cmul(a[2 * r + 1], b[2 + c]));
}
static bool op_1q_matrix(const FusedOp& o, double2 g[4]) {   // uncontrolled 1q op -> its 2x2
  if (o.kind == TG_PHASE && o.nbits == 1) {
    g[0] = make_double2(1, 0); g[1] = g[2] = make_double2(0, 0); g[3] = o.m[0];
    return true;
  }
  if ((o.kind == TG_DENSE1 || o.kind == TG_ANTI1 || o.kind == TG_SWAP1) && o.control < 0) {
    for (int i = 0; i < 4; ++i) g[i] = o.m[i];
    return true;
  }
  return false;
}

// The case an op gets once its register positions are known depends only on its kind and matrix:
// family entry and matrix doubles of the record (tile_kernel.h, record stream).
struct OpShape { int family; int nd; };
// one phase: -1 / i / -i have their own families (2 / 3 / 3 vector instructions per register instead of 4)
static int phase_family(double2 v) {
  const bool sp = tuning().tile_special;
  return (sp && v.x == -1 && v.y == 0) ? OPC_PHASE_NEG : (sp && v.x == 0 && v.y == 1) ? OPC_PHASE_I
         : (sp && v.x == 0 && v.y == -1) ? OPC_PHASE_NI : OPC_PHASE;
}
static OpShape op_shape(const FusedOp& o) {
  const bool sp = tuning().tile_special;
  auto is = [&](int e, double re, double im) { return o.m[e].x == re && o.m[e].y == im; };
  switch (o.kind) {
    case TG_SWAP1: return {OPC_SWAP1, 0};
    case TG_PHASE: {
      const int fam = phase_family(o.m[0]);
      return {fam, fam == OPC_PHASE ? 2 : 0};
    }
    case TG_ANTI1: return (sp && is(1, 0, -1) && is(2, 0, 1)) ? OpShape{OPC_YLIKE1, 0} : OpShape{OPC_ANTI1, 4};
    case TG_DENSE2: return {OPC_DENSE2, 32};
    default:   // a real 2x2 (H, RY, G) needs four doubles instead of eight; an uncontrolled c [[1,1],[1,-1]] none
      if (sp && tuning().tile_had && o.control < 0 && o.m[0].y == 0 && o.m[1].y == 0 && o.m[2].y == 0 && o.m[3].y == 0 &&
          o.m[0].x == o.m[1].x && o.m[0].x == o.m[2].x && o.m[0].x == -o.m[3].x && o.m[0].x != 0)
        return {OPC_HAD1, 0};
      return (sp && o.m[0].y == 0 && o.m[1].y == 0 && o.m[2].y == 0 && o.m[3].y == 0) ? OpShape{OPC_REAL1, 4}
                                                                                        : OpShape{OPC_DENSE1, 8};
  }
}

// vector instructions per thread of the uncontrolled record
static int op_cost(const FusedOp& o) {
  switch (op_shape(o).family) {
    case OPC_PHASE_NEG: return 8;
    case OPC_PHASE: case OPC_HAD1: return 16;
    case OPC_PHASE_I: case OPC_PHASE_NI: return 20;
    case OPC_SWAP1: case OPC_REAL1: return 32;
    case OPC_ANTI1: case OPC_YLIKE1: return 40;
    case OPC_DENSE1: return 68;
    default: return 144;
  }
}
constexpr int kRecordCost = 8;                 // a record's fetch + dispatch, in the same unit

// A real 2x2 [[m0, m1], [m2, m3]] as a unit-diagonal butterfly (OPC_UNIT1): |m0| == |m3| and |m1| == |m2| bitwise -- RY and
// what the rewrite makes of it with an X, Y or Z -- and not the Hadamard shape, which OPC_HAD1 has.  The larger of m0, m1 is
// taken out as s (it joins the pass factor); the ratios that stay have magnitude <= 1 and the fourth one is +-1 EXACTLY:
//   form D, |m0| >= |m1|: s = m0, p = m1 / m0, q = m2 / m0, sigma = m3 / m0   a' = a + p b,  b' = q a + sigma b
//   form A, otherwise:    s = m1, p = m0 / m1, q = m3 / m1, sigma = m2 / m1   a' = p a + b,  b' = sigma a + q b
struct UnitReal { bool form_a, neg; double s, p, q; };
static bool unit_real_of(const double m[4], UnitReal* u = nullptr) {
  if (std::fabs(m[0]) != std::fabs(m[3]) || std::fabs(m[1]) != std::fabs(m[2])) return false;
  if (m[0] == m[1] && m[0] == m[2] && m[0] == -m[3]) return false;
  const bool form_a = !(std::fabs(m[0]) >= std::fabs(m[1]));
  const double s = form_a ? m[1] : m[0];
  if (s == 0 || !std::isfinite(s)) return false;
  if (u) {
    u->form_a = form_a;
    u->s = s;
    u->p = (form_a ? m[0] : m[1]) / s;
    u->q = (form_a ? m[3] : m[2]) / s;
    u->neg = std::signbit(form_a ? m[2] : m[3]) != std::signbit(s);
  }
  return true;
}
// The family an uncontrolled op's record is PRICED as: what reaches the device (lower_unit_real, tile_groups.h).
static int priced_family(const FusedOp& o) {
  const int fam = op_shape(o).family;
  if (fam != OPC_REAL1 || !tuning().tile_unit || o.control >= 0) return fam;
  const double m[4] = {o.m[0].x, o.m[1].x, o.m[2].x, o.m[3].x};
  return unit_real_of(m) ? OPC_UNIT1 : fam;
}

// The MEASURED price of the gate engine (runner/engine_cost_model.json, fitted by tools/fit_engine_cost_model.py to one-pass
// probes on MI355X): microseconds a record of each kind adds to a pass of the fitted state size once the pass is past the
// knee -- the engine time a pass hides under its memory time.  Handed in by the caller (QSIM_ENGINE_COST_* of
// include/qsim_hip.h name the entries), never read from the environment; a null table switches every priced decision off.
struct EngineCosts {
  double v[QSIM_ENGINE_COST_COUNT];
  double of_family(int family) const {
    switch (family) {
      case OPC_DENSE1: return v[QSIM_ENGINE_COST_DENSE1];
      case OPC_REAL1: return v[QSIM_ENGINE_COST_REAL1];
      case OPC_HAD1: return v[QSIM_ENGINE_COST_HAD1];
      case OPC_UNIT1: return v[QSIM_ENGINE_COST_UNIT1];
      case OPC_SWAP1: return v[QSIM_ENGINE_COST_SWAP1];
      case OPC_ASWAP1: return v[QSIM_ENGINE_COST_ASWAP1];
      case OPC_ANTI1: case OPC_YLIKE1: return v[QSIM_ENGINE_COST_ANTI1];
      case OPC_PHASE: return v[QSIM_ENGINE_COST_PHASE];
      case OPC_PHASE_NEG: return v[QSIM_ENGINE_COST_PHASE_NEG];
      case OPC_PHASE_I: case OPC_PHASE_NI: return v[QSIM_ENGINE_COST_PHASE_I];
      case OPC_DIAGR: return v[QSIM_ENGINE_COST_DIAGR];
      case OPC_SCALE: return v[QSIM_ENGINE_COST_PHASE];
      default: return v[QSIM_ENGINE_COST_DENSE2];
    }
  }
  // family of a written record's case entry (families are runs of entries: the last base at or below it)
  static int family_of_entry(int opcode) {
    static const int bases[] = {OPC_DENSE1, OPC_SWAP1, OPC_ANTI1, OPC_PHASE, OPC_DENSE2, OPC_REAL1, OPC_YLIKE1, OPC_PHASE_NEG,
                                OPC_PHASE_I, OPC_PHASE_NI, OPC_DIAGR, OPC_HAD1, OPC_SCALE, OPC_ASWAP1, OPC_UNIT1};
    int best = OPC_DENSE1;
    for (int b : bases) if (b <= opcode && b > best) best = b;
    return best;
  }
  // an unconditional real 2x2 of the unit-diagonal family reaches the device as OPC_UNIT1 (lower_unit_real) ...
  static bool lowers_to_unit(const TileDesc& d) {
    return tuning().tile_unit && tuning().tile_special && d.opcode >= OPC_REAL1 && d.opcode < OPC_REAL1 + 3 && !d.blk_mask && !d.outer_mask &&
           unit_real_of(d.m);
  }
  // microseconds of one written record at the fitted state size
  double of_record(const TileDesc& d) const {
    int fam = family_of_entry(d.opcode);
    if (lowers_to_unit(d)) fam = OPC_UNIT1;
    const bool one_q = fam == OPC_DENSE1 || fam == OPC_SWAP1 || fam == OPC_ANTI1 || fam == OPC_REAL1 || fam == OPC_YLIKE1 || fam == OPC_ASWAP1;
    return of_family(fam) * (d.blk_mask ? v[QSIM_ENGINE_COST_PRED_LANE] : 1.0) * (d.outer_mask ? v[QSIM_ENGINE_COST_PRED_OUTER] : 1.0) *
           ((one_q && d.opcode - fam >= 3) ? v[QSIM_ENGINE_COST_REG_CTRL] : 1.0);
  }
  // modelled engine microseconds of a pass on 2^k amplitudes
  double of_pass(const std::vector<TileGroup>& groups, int k) const {
    double us = v[QSIM_ENGINE_COST_FIXED_US];
    if (!groups.empty() && tuning().tile_direct)          // (full tiles: an end above the line bits skips its LDS trip)
      us += v[QSIM_ENGINE_COST_DIRECT_END] * ((groups.front().s[0] >= kTileLow) + (groups.back().s[0] >= kTileLow));
    bool host = false, unit = false;     // ... except one that has to carry the factors: a pass with no other record to fold them into
    for (const TileGroup& g : groups) {
      us += v[QSIM_ENGINE_COST_GROUP];
      for (const TileDesc& d : g.gates) {
        us += of_record(d);
        if (lowers_to_unit(d)) unit = true;
        else if (factor_host_doubles(d.opcode) && !d.blk_mask && !d.outer_mask) host = true;
      }
    }
    if (unit && !host) us += v[QSIM_ENGINE_COST_REAL1] - v[QSIM_ENGINE_COST_UNIT1];
    return us * std::ldexp(1.0, k - (int)v[QSIM_ENGINE_COST_FIT_QUBITS]);
  }
};
// (false: no table, pricing off)
static bool engine_costs_from(const double* table, int count, EngineCosts* ec) {
  if (!table || count < QSIM_ENGINE_COST_COUNT) return false;
  for (int i = 0; i < QSIM_ENGINE_COST_COUNT; ++i) ec->v[i] = table[i];
  return true;
}

// ---- commutation-aware fusion of one-qubit gates -------------------------------------------------
// The host planners (circuit/fusion.py, the reference's fuse_1q_ops) only merge 1q gates that are ADJACENT on their
// qubit.  Inside the library a 1q gate G on qubit q also moves forward past every op it commutes with -- a
// controlled gate whose control is q when G is diagonal (Z, S, T, R), a controlled gate whose target is q when G
// commutes with its 2x2 (X through CNOT targets), a CZ / CR on q when G is diagonal -- and is multiplied into the
// next 1q gate on q.  Same unitary (rounding differs at 1e-16); on the bench circuit 1 in 5 1q gates disappears
// this way, among them every X (the costliest 1q record of the engine: 16 v_swap_b32 at half rate).
static void commute_fuse_1q(std::vector<FusedOp>* ops, bool backward) {
  // forward: gate i moves later, into the next 1q gate j on its qubit (the product sits at j); backward: that gate j
  // moves earlier, into i (the product sits at i) -- legal under the same condition, everything between them on the
  // qubit commuting with the gate that moves... which for the backward form is gate j: its matrix is the one tested.
  const size_t n = ops->size();
  std::vector<char> dead(n, 0);
  constexpr size_t kWindow = 512;              // ops looked at behind a gate (bounds the cost on long lists)
  auto zero = [](double2 v) { return v.x == 0 && v.y == 0; };
  auto commutes_with = [&](const double2 g[4], const FusedOp& o, int q) {
    const bool diag = zero(g[1]) && zero(g[2]);
    if (o.kind == TG_PHASE) return diag;                                   // CZ / CR
    if (o.kind == TG_DENSE2) return false;
    if (o.control == q) return diag;                                       // q controls it
    if (o.control >= 0 && o.target[0] == q) {                              // q is its target: g v == v g ?
      double2 gv[4], vg[4];
      mul2x2(g, o.m, gv);
      mul2x2(o.m, g, vg);
      for (int e = 0; e < 4; ++e)
        if (gv[e].x != vg[e].x || gv[e].y != vg[e].y) return false;
      return true;
    }
    return false;
  };
  for (size_t i = 0; i < n; ++i) {
    double2 g[4];
    if (dead[i] || !op_1q_matrix((*ops)[i], g)) continue;
    const int q = (*ops)[i].qubits[0];
    // the next 1q gate j on q, and whether everything on q in between commutes with the gate that moves
    size_t j = i + 1;
    bool g_passes = true, found = false;
    std::vector<size_t> between;
    for (; j < n && j <= i + kWindow; ++j) {
      const FusedOp& o = (*ops)[j];
      if (dead[j] || !((op_qmask(o) >> q) & 1)) continue;
      double2 h[4];
      if (op_1q_matrix(o, h)) { found = true; break; }
      between.push_back(j);
      if (!backward && !commutes_with(g, o, q)) { g_passes = false; break; }
    }
    if (!found || !g_passes) continue;
    double2 h[4];
    op_1q_matrix((*ops)[j], h);
    if (backward) {
      bool ok = true;
      for (size_t b : between) ok = ok && commutes_with(h, (*ops)[b], q);
      if (!ok) continue;
    }
    double2 f[4];
    mul2x2(h, g, f);
    const double U[8] = {f[0].x, f[0].y, f[1].x, f[1].y, f[2].x, f[2].y, f[3].x, f[3].y};
    const int32_t qq[2] = {q, -1};
    auto frac = [](const FusedOp& x) { return x.absorbed + 1.0 / (double)(1ull << (x.kind == TG_PHASE ? x.nbits : x.halvings)); };
    const size_t keep = backward ? i : j, drop = backward ? j : i;
    const double moved = (*ops)[keep].absorbed + frac((*ops)[drop]);
    FusedOp fused;
    const bool identity = !classify_op(1, qq, U, &fused);
    // Worth it?  The engine's special cases are cheap (Z 8, H 16, T 16, S 20 vector instructions per thread against 32
    // for a real 2x2, 40 anti-diagonal, 68 complex): a product that costs more than its factors plus one record's
    // dispatch is left alone (measured: fusing everything that commutes made the pass 2 % slower at 15 % fewer records).
    if (!identity && op_cost(fused) > op_cost((*ops)[i]) + op_cost((*ops)[j]) + kRecordCost) continue;
    if (!identity) { fused.absorbed = moved; (*ops)[keep] = fused; }
    else dead[keep] = 1;                        // the product is the identity
    dead[drop] = 1;
    if (backward && !dead[i]) --i;              // the product may take the next gate in as well
  }
  size_t w = 0;
  for (size_t i = 0; i < n; ++i) if (!dead[i]) (*ops)[w++] = (*ops)[i];
  ops->resize(w);
}

// The op list a builder plans: the caller's, after the library-side fusion of commuting 1q gates (off by default).
static std::vector<FusedOp> planned_ops(const std::vector<FusedOp>& ops_in) {
  const Tuning& tune = tuning();
  std::vector<FusedOp> ops = ops_in;
  if (tune.tile_commute_fuse == 1 || tune.tile_commute_fuse == 4) commute_fuse_1q(&ops, false);
  if (tune.tile_commute_fuse >= 2) commute_fuse_1q(&ops, true);
  if (tune.tile_commute_fuse == 3) commute_fuse_1q(&ops, false);
  return ops;
}

// hash of a byte string: the plan cache's key (tile_launch.h) and the done-sets of the searching builder (tile_search.h)
static u64 fnv1a(const unsigned char* p, size_t n, u64 h = 1469598103934665603ull) {
  for (size_t i = 0; i < n; ++i) { h ^= p[i]; h *= 1099511628211ull; }
  return h;
}
