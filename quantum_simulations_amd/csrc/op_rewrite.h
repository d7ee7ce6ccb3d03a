// op_rewrite.h -- host-side rewrite of an op list before it is planned: what the planner is given.
// Part of the single translation unit qsim_hip.hip (included there, in order; not a standalone header).
//
// The pass count of a fused plan follows from how many ops need their TARGET qubit inside the tile (diagonal ops and
// controls run from outside as predicates).  Two families of such needs can be rewritten away exactly:
//   (a) CNOT(c,t) next to an H on t:  CNOT H_t = H_t CZ,  H_t CNOT = CZ H_t.  The CNOT becomes a CZ (diagonal), the H moves
//       to the other side and multiplies into the neighbouring 1q gate on t.
//   (b) X and Y (any anti-diagonal 2x2 A = X D): an X is a bit flip of the index.  It is kept as one pending bit per qubit
//       (the "frame") and pushed forward: it conjugates a diagonal into a diagonal, passes a CNOT target, spreads through a
//       CNOT control, leaves a phase at a CZ / CR, changes sides at a SWAP and is absorbed by the next dense 1q gate (G X
//       is still one 2x2) or dense 2q gate (a permutation of its columns).  A controlled 2x2 lets it pass on the target
//       (C(V) -> C(X V X)) and takes it in on the control (the op becomes a dense 2q gate).
//   (c) what is still pending at the end of the list is pushed BACKWARDS by the mirrored rules into the nearest earlier
//       dense gate (X G); a frame that reaches the front of the list becomes an explicit X there.
//   (d) (priced calls only) a diagonal 1q gate D is multiplied into a dense 1q gate U on its qubit -- U D when U comes later,
//       D U when it came before -- when only ops that are diagonal on that qubit (controls, CZ / CR, other diagonals: they
//       commute with D) lie between them and the engine cost table prices the product's record below the two it replaces: Z
//       always pays, S or T make a complex 2x2 of a real one and pay only where that is cheaper.  The dense gate stays where
//       it is, so no op that needs a tile appears or moves.
// All identities are algebraic: they hold for non-unitary factors (collapse factors) and drop no global phase -- a diagonal
// diag(d0, d1) that a frame leaves behind is written as the phase gate diag(1, d1 / d0), which needs no tile, and the
// factor d0 is multiplied into one dense 1q gate of the list.  Same amplitudes up to the rounding of the 2x2 products.
// Classification ("diagonal", "is exactly CNOT / CZ") is classify_op's, by exact entries, as everywhere in the planner.
struct RwOp {
  int nq;
  int32_t q[2];
  double U[32];
  FusedOp f;
};

enum RwClass { RW_DIAG1, RW_ANTI1, RW_DENSE1, RW_CNOT, RW_PHASE2, RW_SWAP2, RW_OTHER };

static inline bool rw_zero(double2 v) { return v.x == 0 && v.y == 0; }
static inline bool rw_is_one(double2 v) { return v.x == 1 && v.y == 0; }
static inline double2 rw_div(double2 a, double2 b) {
  const double d = b.x * b.x + b.y * b.y;
  return make_double2((a.x * b.x + a.y * b.y) / d, (a.y * b.x - a.x * b.y) / d);
}

static RwClass rw_class(const RwOp& o) {
  const FusedOp& f = o.f;
  if (f.kind == TG_PHASE) return f.nbits == 1 ? RW_DIAG1 : (rw_zero(f.m[0]) ? RW_OTHER : RW_PHASE2);
  if (f.kind == TG_DENSE2) return f.halvings == 1 ? RW_SWAP2 : RW_OTHER;
  if (f.control >= 0) return f.kind == TG_SWAP1 ? RW_CNOT : RW_OTHER;
  if (f.kind == TG_ANTI1 || f.kind == TG_SWAP1) return RW_ANTI1;
  return (rw_zero(f.m[1]) && rw_zero(f.m[2])) ? RW_DIAG1 : RW_DENSE1;
}
// does the op act as a diagonal matrix on qubit q (a 1q diagonal, a control, a phase bit)?
static bool rw_diagonal_on(const RwOp& o, int q) {
  const FusedOp& f = o.f;
  if (f.kind == TG_PHASE) return true;
  if (f.kind == TG_DENSE2) return false;
  if (f.control >= 0) return q == f.control;
  return rw_zero(f.m[1]) && rw_zero(f.m[2]);
}
static inline bool rw_needs_tile(const RwOp& o) { return o.f.ntargets > 0; }

// an uncontrolled 1q op from its 2x2; false: the identity
static bool rw_make_1q(int q, const double2 g[4], RwOp* o) {
  std::memset(o->U, 0, sizeof o->U);
  for (int i = 0; i < 4; ++i) { o->U[2 * i] = g[i].x; o->U[2 * i + 1] = g[i].y; }
  o->nq = 1;
  o->q[0] = q;
  o->q[1] = 0;
  return classify_op(1, o->q, o->U, &o->f);
}
static bool rw_make_phase2(int a, int b, double2 p, RwOp* o) {   // diag(1, 1, 1, p); false: the identity
  std::memset(o->U, 0, sizeof o->U);
  o->U[0] = o->U[10] = o->U[20] = 1.0;
  o->U[30] = p.x; o->U[31] = p.y;
  o->nq = 2;
  o->q[0] = a; o->q[1] = b;
  return classify_op(2, o->q, o->U, &o->f);
}
static void rw_1q_matrix(const RwOp& o, double2 g[4]) { op_1q_matrix(o.f, g); }
// exactly the Hadamard matrix (1/sqrt(2) to the last bit, either rounding of it)
static bool rw_is_h(const RwOp& o) {
  if (rw_class(o) != RW_DENSE1) return false;
  const double2* m = o.f.m;
  if (m[0].y != 0 || m[1].y != 0 || m[2].y != 0 || m[3].y != 0) return false;
  if (!(m[0].x == m[1].x && m[0].x == m[2].x && m[0].x == -m[3].x)) return false;
  return std::fabs(m[0].x - 0.70710678118654752440) <= 1.2e-16;
}

// ---- (a) CNOT with an exact H next to it on the target -> CZ --------------------------------------------------------
static void rw_h_conversion(const std::vector<RwOp>& list, std::vector<RwOp>* result, int n_qubits) {
  std::vector<RwOp> in = list;
  const size_t n = in.size();
  std::vector<char> in_dead(n, 0);
  std::vector<long> nxt(2 * n, -1);               // nxt[2 i + s]: the next input op on qubit in[i].q[s]
  {
    std::vector<long> seen((size_t)n_qubits, -1);
    for (size_t i = n; i-- > 0;)
      for (int s = 0; s < in[i].nq; ++s) { nxt[2 * i + s] = seen[(size_t)in[i].q[s]]; seen[(size_t)in[i].q[s]] = (long)i; }
  }
  auto next_on = [&](size_t i, int q) {
    long j = (long)i;
    do {
      const RwOp& o = in[(size_t)j];
      j = nxt[2 * (size_t)j + ((o.nq == 2 && o.q[1] == q) ? 1 : 0)];
    } while (j >= 0 && in_dead[(size_t)j]);
    return j;
  };
  std::vector<RwOp>& out = *result;
  out.clear();
  out.reserve(n + 8);
  std::vector<char> dead;
  std::vector<long> prv;                          // prv[2 i + s]: the op of `out` before out[i] on its qubit s
  std::vector<long> last((size_t)n_qubits, -1);
  auto push = [&](const RwOp& o) {
    const long at = (long)out.size();
    out.push_back(o);
    dead.push_back(0);
    prv.push_back(-1); prv.push_back(-1);
    for (int s = 0; s < o.nq; ++s) { prv[2 * (size_t)at + s] = last[(size_t)o.q[s]]; last[(size_t)o.q[s]] = at; }
  };
  auto drop_last_1q = [&](int q) {                // the last op on q is an uncontrolled 1q op: take it out
    const long p = last[(size_t)q];
    dead[(size_t)p] = 1;
    last[(size_t)q] = prv[2 * (size_t)p];
  };
  auto is_1q = [&](const RwOp& o) { const RwClass c = rw_class(o); return c == RW_DIAG1 || c == RW_ANTI1 || c == RW_DENSE1; };
  for (size_t i = 0; i < n; ++i) {
    if (in_dead[i]) continue;
    const RwOp& o = in[i];
    if (rw_class(o) != RW_CNOT) { push(o); continue; }
    const int c = o.f.control, t = o.f.target[0];
    RwOp cz;
    rw_make_phase2(c, t, make_double2(-1.0, 0.0), &cz);
    const long p = last[(size_t)t];
    if (p >= 0 && rw_is_h(out[(size_t)p])) {      // H_t then CNOT  =  CZ then H_t
      const RwOp h = out[(size_t)p];
      drop_last_1q(t);
      push(cz);
      const long j = next_on(i, t);
      if (j >= 0 && is_1q(in[(size_t)j])) {
        if (rw_is_h(in[(size_t)j])) { in_dead[(size_t)j] = 1; continue; }          // H H = 1, exactly
        double2 g[4], hm[4], prod[4];
        rw_1q_matrix(in[(size_t)j], g);
        rw_1q_matrix(h, hm);
        mul2x2(g, hm, prod);
        if (!rw_make_1q(t, prod, &in[(size_t)j])) in_dead[(size_t)j] = 1;
      } else {
        push(h);
      }
      continue;
    }
    const long j = next_on(i, t);
    if (j >= 0 && rw_is_h(in[(size_t)j])) {       // CNOT then H_t  =  H_t then CZ
      const RwOp h = in[(size_t)j];
      in_dead[(size_t)j] = 1;
      if (p >= 0 && is_1q(out[(size_t)p])) {
        double2 g[4], hm[4], prod[4];
        rw_1q_matrix(out[(size_t)p], g);
        rw_1q_matrix(h, hm);
        mul2x2(hm, g, prod);
        RwOp fused;
        if (rw_make_1q(t, prod, &fused)) { fused.f.absorbed = 0; out[(size_t)p] = fused; }
        else drop_last_1q(t);
      } else {
        push(h);
      }
      push(cz);
      continue;
    }
    push(o);
  }
  size_t w = 0;
  for (size_t i = 0; i < out.size(); ++i) if (!dead[i]) { if (w != i) out[w] = out[i]; ++w; }
  out.resize(w);
}

// ---- (b), (c) the X frame, forwards or backwards ----------------------------------------------------------------------
// `frame`: in, the pending X per qubit where the sweep starts; out, what is pending where it ends (forwards: the end of the
// list; backwards: nothing, the front of the list got explicit X ops).  `scalar` collects the factors taken out of
// conjugated diagonals.
static void rw_frame_sweep(const std::vector<RwOp>& in, bool backward, std::vector<char>* frame_io, double2* scalar,
                           std::vector<RwOp>* result, int n_qubits) {
  std::vector<char>& frame = *frame_io;
  std::vector<RwOp>& out = *result;
  const size_t n = in.size();
  out.clear();
  out.reserve(n + 8);
  const double2 X[4] = {make_double2(0, 0), make_double2(1, 0), make_double2(1, 0), make_double2(0, 0)};
  // forwards only: an X that nothing precedes on its qubit and that nothing later on its qubit would absorb stays where it
  // is -- it is where the backward flush would put it again
  std::vector<char> open_tail(n, 0);
  if (!backward) {
    std::vector<char> free_to_end((size_t)n_qubits, 1);
    for (size_t i = n; i-- > 0;) {
      const RwClass c = rw_class(in[i]);
      if (c == RW_ANTI1) open_tail[i] = free_to_end[(size_t)in[i].q[0]];
      const bool passes = c == RW_DIAG1 || c == RW_CNOT || c == RW_PHASE2;
      if (c == RW_SWAP2) std::swap(free_to_end[(size_t)in[i].q[0]], free_to_end[(size_t)in[i].q[1]]);
      else if (c == RW_OTHER && in[i].f.control >= 0) free_to_end[(size_t)in[i].f.control] = 0;   // (its target lets an X pass)
      else if (!passes) for (int s = 0; s < in[i].nq; ++s) free_to_end[(size_t)in[i].q[s]] = 0;
    }
  }
  std::vector<long> last_diag((size_t)n_qubits, -1);        // the diagonal 1q gate written on a qubit since the last op that is not diagonal on it
  std::vector<char> gone;                                   // written ops that were multiplied into a later one
  auto put = [&](const RwOp& o) {
    for (int s = 0; s < o.nq; ++s)
      if (!rw_diagonal_on(o, o.q[s])) last_diag[(size_t)o.q[s]] = -1;
    out.push_back(o);
    gone.push_back(0);
  };
  std::vector<char> before((size_t)n_qubits, 0);            // an op precedes on the qubit
  // diag(d0, d1) on q; normalise: as a phase gate diag(1, d1 / d0) and a factor
  auto put_diag = [&](int q, double2 d0, double2 d1, bool normalise) {
    double2 g[4] = {d0, make_double2(0, 0), make_double2(0, 0), d1};
    if (normalise && !rw_is_one(d0) && !rw_zero(d0)) {
      *scalar = cmul(*scalar, d0);
      g[0] = make_double2(1, 0);
      g[3] = rw_div(d1, d0);
    }
    // ... multiplied into the diagonal 1q gate the sweep wrote on q before, when only ops that are diagonal on q (controls,
    // CZ / CR: they commute with it) came between them
    const long at = last_diag[(size_t)q];
    if (at >= 0) {
      double2 h[4];
      rw_1q_matrix(out[(size_t)at], h);
      g[0] = cmul(g[0], h[0]);
      g[3] = cmul(g[3], h[3]);
      gone[(size_t)at] = 1;
    }
    RwOp o;
    if (rw_make_1q(q, g, &o)) { put(o); last_diag[(size_t)q] = (long)out.size() - 1; }
    else last_diag[(size_t)q] = -1;
  };
  auto emit_diag = [&](int q, double2 d0, double2 d1) { put_diag(q, d0, d1, true); };
  auto explicit_x = [&](int q) {
    RwOp o;
    rw_make_1q(q, X, &o);
    put(o);
  };
  for (size_t step = 0; step < n; ++step) {
    const size_t i = backward ? n - 1 - step : step;
    const RwOp& o = in[i];
    const RwClass c = rw_class(o);
    const int q0 = o.q[0];
    double2 g[4];
    switch (c) {
      case RW_DIAG1:
        rw_1q_matrix(o, g);
        if (frame[(size_t)q0]) emit_diag(q0, g[3], g[0]);
        else put_diag(q0, g[0], g[3], false);
        break;
      case RW_ANTI1:
        rw_1q_matrix(o, g);
        if (frame[(size_t)q0]) {                            // A X (X A backwards) is diagonal
          if (backward) emit_diag(q0, g[2], g[1]); else emit_diag(q0, g[1], g[2]);
          frame[(size_t)q0] = 0;
        } else if (backward || (o.f.kind == TG_SWAP1 && !before[(size_t)q0] && open_tail[i])) {
          put(o);
        } else {                                            // A = X (X A): the diagonal now, the X pending
          emit_diag(q0, g[2], g[1]);
          frame[(size_t)q0] = 1;
        }
        break;
      case RW_DENSE1:
        if (frame[(size_t)q0]) {
          rw_1q_matrix(o, g);
          const double2 gx[4] = {g[1], g[0], g[3], g[2]}, xg[4] = {g[2], g[3], g[0], g[1]};
          RwOp fused;
          if (rw_make_1q(q0, backward ? xg : gx, &fused)) put(fused);
          frame[(size_t)q0] = 0;
        } else {
          put(o);
        }
        break;
      case RW_CNOT:
        put(o);
        frame[(size_t)o.f.target[0]] ^= frame[(size_t)o.f.control];
        break;
      case RW_SWAP2:
        put(o);
        std::swap(frame[(size_t)o.q[0]], frame[(size_t)o.q[1]]);
        break;
      case RW_PHASE2: {                                     // CZ / CR: X_a CP(p) X_a = P_b(p) CP(1/p)
        const int a = o.f.bits[0], b = o.f.bits[1];
        const double2 p = o.f.m[0], one = make_double2(1, 0);
        const bool fa = frame[(size_t)a], fb = frame[(size_t)b];
        if (!fa && !fb) { put(o); break; }
        RwOp cp;
        if (fa && fb) {
          put(o);
          *scalar = cmul(*scalar, p);
          emit_diag(a, one, rw_div(one, p));
          emit_diag(b, one, rw_div(one, p));
        } else {
          if (rw_make_phase2(a, b, rw_div(one, p), &cp)) put(cp);
          emit_diag(fa ? b : a, one, p);
        }
        break;
      }
      default: {                                            // dense 2q, controlled 2x2: the X goes into the 4x4
        const int fa = frame[(size_t)o.q[0]], fb = frame[(size_t)o.q[1]];
        if (!fa && !fb) { put(o); break; }
        // a controlled V with the X on its target only: X C(V) X = C(X V X), the frame stays; everything else takes the
        // pending X of its qubits in as a permutation of its columns (rows backwards) and ends them
        const bool through = o.f.control >= 0 && !frame[(size_t)o.f.control];
        const int mask = 2 * fa + fb;
        RwOp u = o;
        for (int r = 0; r < 4; ++r)
          for (int col = 0; col < 4; ++col) {
            const int from = through ? 4 * (r ^ mask) + (col ^ mask) : (backward ? 4 * (r ^ mask) + col : 4 * r + (col ^ mask));
            u.U[2 * (4 * r + col)] = o.U[2 * from];
            u.U[2 * (4 * r + col) + 1] = o.U[2 * from + 1];
          }
        if (classify_op(2, u.q, u.U, &u.f)) put(u);
        if (!through) frame[(size_t)o.q[0]] = frame[(size_t)o.q[1]] = 0;
        break;
      }
    }
    for (int s = 0; s < o.nq; ++s) before[(size_t)o.q[s]] = 1;
  }
  if (backward) {
    for (int q = n_qubits; q-- > 0;)
      if (frame[(size_t)q]) { explicit_x(q); frame[(size_t)q] = 0; }
  }
  size_t w = 0;
  for (size_t i = 0; i < out.size(); ++i) if (!gone[i]) { if (w != i) out[w] = out[i]; ++w; }
  out.resize(w);
  if (backward) std::reverse(out.begin(), out.end());
}

// ---- (d) a diagonal 1q gate into a dense 1q gate on its qubit ------------------------------------------------------------------
static double rw_record_us(const EngineCosts& ec, const RwOp& o) { return ec.of_family(priced_family(o.f)); }
// one sweep; true: something was merged (a host that turned complex takes further diagonals in for nothing: sweep again)
static bool rw_merge_diagonals(std::vector<RwOp>* list, int n_qubits, const EngineCosts& ec) {
  std::vector<RwOp>& ops = *list;
  const size_t n = ops.size();
  std::vector<char> dead(n, 0);
  std::vector<std::vector<size_t>> on((size_t)n_qubits);      // the ops on every qubit, in list order
  for (size_t i = 0; i < n; ++i)
    for (int s = 0; s < ops[i].nq; ++s) on[(size_t)ops[i].q[s]].push_back(i);
  bool any = false;
  for (int q = 0; q < n_qubits; ++q) {
    const std::vector<size_t>& w = on[(size_t)q];
    for (size_t a = 0; a < w.size(); ++a) {
      const size_t i = w[a];
      if (dead[i] || rw_class(ops[i]) != RW_DIAG1) continue;
      // the nearest op on q that is not diagonal on q, later [0] and earlier [1]: a host when it is a dense 1q gate
      long host[2] = {-1, -1};
      for (size_t b = a + 1; b < w.size(); ++b) {
        if (dead[w[b]] || rw_diagonal_on(ops[w[b]], q)) continue;
        if (rw_class(ops[w[b]]) == RW_DENSE1) host[0] = (long)w[b];
        break;
      }
      for (size_t b = a; b-- > 0;) {
        if (dead[w[b]] || rw_diagonal_on(ops[w[b]], q)) continue;
        if (rw_class(ops[w[b]]) == RW_DENSE1) host[1] = (long)w[b];
        break;
      }
      double2 d[4];
      rw_1q_matrix(ops[i], d);
      double best_gain = 0;
      int best = -1;
      RwOp merged[2];
      bool identity[2] = {false, false};
      for (int side = 0; side < 2; ++side) {
        if (host[side] < 0) continue;
        double2 u[4], prod[4];
        rw_1q_matrix(ops[(size_t)host[side]], u);
        if (side == 0) mul2x2(u, d, prod); else mul2x2(d, u, prod);
        identity[side] = !rw_make_1q(q, prod, &merged[side]);
        const double gain = rw_record_us(ec, ops[i]) + rw_record_us(ec, ops[(size_t)host[side]]) -
                            (identity[side] ? 0.0 : rw_record_us(ec, merged[side]));
        if (gain > best_gain) { best_gain = gain; best = side; }
      }
      if (best < 0) continue;
      if (identity[best]) dead[(size_t)host[best]] = 1; else ops[(size_t)host[best]] = merged[best];
      dead[i] = 1;
      any = true;
    }
  }
  size_t w = 0;
  for (size_t i = 0; i < n; ++i) if (!dead[i]) { if (w != i) ops[w] = ops[i]; ++w; }
  ops.resize(w);
  return any;
}

// One application of (a), (b), (c) and, with a cost table, (d).  When the factor taken out of the diagonals finds no dense 1q gate to go into (a list
// without one), the list after (a) is the result.
static void rw_once(const std::vector<RwOp>& in, int n_qubits, std::vector<RwOp>* out, const EngineCosts* ec) {
  std::vector<RwOp> a, b, c;
  rw_h_conversion(in, &a, n_qubits);
  std::vector<char> frame((size_t)n_qubits, 0);
  double2 scalar = make_double2(1, 0);
  rw_frame_sweep(a, false, &frame, &scalar, &b, n_qubits);
  rw_frame_sweep(b, true, &frame, &scalar, &c, n_qubits);
  if (!rw_is_one(scalar)) {
    // a factor commutes with everything: into one uncontrolled dense 1q gate -- a complex 2x2 when there is one (a real
    // 2x2 and the Hadamard have cheaper records, which a complex factor would cost them), else a real one, else any
    const bool real = scalar.y == 0;
    long host = -1;
    int best = 0;
    for (size_t i = 0; i < c.size() && best < 3; ++i) {
      if (rw_class(c[i]) != RW_DENSE1) continue;
      const double2* m = c[i].f.m;
      const bool cplx = m[0].y != 0 || m[1].y != 0 || m[2].y != 0 || m[3].y != 0;
      const int rank = cplx ? 3 : (real && !rw_is_h(c[i])) ? 2 : 1;
      if (rank > best) { best = rank; host = (long)i; }
    }
    if (host < 0) {
      c = a;
    } else {
      double2 g[4];
      rw_1q_matrix(c[(size_t)host], g);
      for (int e = 0; e < 4; ++e) g[e] = cmul(scalar, g[e]);
      RwOp scaled;
      rw_make_1q(c[(size_t)host].q[0], g, &scaled);
      c[(size_t)host] = scaled;
    }
  }
  if (ec) while (rw_merge_diagonals(&c, n_qubits, *ec)) {}
  *out = c;
}

static int rw_need_tile(const std::vector<RwOp>& ops) {
  int need = 0;
  for (const RwOp& o : ops) need += rw_needs_tile(o);
  return need;
}

// The rewritten list of a checked op list (identities drop out).  One application of the rules is no canonical form: an X
// that spreads through CNOT controls on its way can leave more explicit X ops at the front of the list than it removes, and
// a second application may find a dense gate for an X the first one left at the front.  So the rules are applied again as
// long as the list gets better -- fewer ops that need a tile, or as many and fewer ops -- and the last list that was an
// improvement is the result: never more tile needs than the caller's list, and a rewritten list is a fixed point.
static void rewrite_op_list(int n_qubits, int n_ops, const int32_t* nq, const int32_t* qubits, const double* mats,
                            std::vector<RwOp>* out, int* need_tile_in, const EngineCosts* ec = nullptr) {
  std::vector<RwOp> cur;
  cur.reserve((size_t)n_ops);
  for (int i = 0; i < n_ops; ++i) {
    RwOp o;
    o.nq = nq[i];
    o.q[0] = qubits[2 * i];
    o.q[1] = nq[i] == 2 ? qubits[2 * i + 1] : 0;
    std::memset(o.U, 0, sizeof o.U);
    std::memcpy(o.U, mats + 32 * (size_t)i, sizeof(double) * (nq[i] == 1 ? 8 : 32));
    if (classify_op(o.nq, o.q, o.U, &o.f)) cur.push_back(o);
  }
  int need = rw_need_tile(cur);
  if (need_tile_in) *need_tile_in = need;
  for (int round = 0; round < 8; ++round) {
    std::vector<RwOp> next;
    rw_once(cur, n_qubits, &next, ec);
    const int need_next = rw_need_tile(next);
    if (need_next > need || (need_next == need && next.size() >= cur.size())) break;
    cur.swap(next);
    need = need_next;
  }
  out->swap(cur);
}
