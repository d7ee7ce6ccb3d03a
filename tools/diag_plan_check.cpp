// Stand-alone host check of quantum_simulations_amd/csrc/diag_plan.h: the argument checks, the sort by inner mask, the
// segment cut into pieces and joins -- and, on top of the tables, a host restatement of what k_diag_tile does with them
// per tile (pieces, joins, unscaled Walsh-Hadamard transform) against the direct sum; the same for the per-term values
// (diag_value_table, a host restatement of k_diag_term_values and the row sum).  No GPU, no HIP.  Meant for the
// host sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/diag_plan_check.cpp -o diag_plan_check && ./diag_plan_check
// Exit status 0 and a last line "diag_plan_check: ok" mean that every case passed.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <vector>

typedef unsigned long long u64;
enum { QSIM_OK = 0, QSIM_ERR_INVALID = -1, QSIM_ERR_NONLOCAL = -2 };
static std::string g_err;
static int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}
constexpr int kExpTileBits = 11;

#include "../quantum_simulations_amd/csrc/diag_plan.h"

static int g_failed = 0;
#define CHECK(cond)                                                              \
  do {                                                                           \
    if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_failed; } \
  } while (0)

// the tables' invariants for a list of n terms on tiles of tb bits
static void check_tables(int tb, int n, const std::vector<uint64_t>& z, const std::vector<double>& c, const DiagTable& d) {
  const u64 inner = (1ull << tb) - 1;
  CHECK((int)d.terms.size() == n);
  std::vector<int> covered((size_t)n, 0);
  int slots = 0;
  size_t join = 0;
  long prev_zi = -1;
  for (size_t p = 0; p < d.pieces.size(); ++p) {
    const DiagPiece& pc = d.pieces[p];
    CHECK(pc.count >= 1 && pc.count <= kDiagPiece && pc.first >= 0 && pc.first + pc.count <= n);
    CHECK(pc.zi <= inner && (long)pc.zi >= prev_zi);
    for (int i = 0; i < pc.count; ++i) ++covered[(size_t)(pc.first + i)];
    if (pc.slot >= 0) {
      CHECK(pc.slot == slots);
      ++slots;
      CHECK(join < d.joins.size());
      if (join < d.joins.size()) {
        const DiagJoin& j = d.joins[join];
        CHECK(j.zi == pc.zi && pc.slot >= j.slot && pc.slot < j.slot + j.count && j.count >= 2);
        if (pc.slot == j.slot + j.count - 1) ++join;
      }
    } else {
      CHECK((long)pc.zi > prev_zi);                 // a whole segment: its zi appears once
    }
    prev_zi = (long)pc.zi;
  }
  CHECK(join == d.joins.size() && slots == d.n_slots && d.n_slots <= kDiagMaxSlots);
  for (int i = 0; i < n; ++i) CHECK(covered[(size_t)i] == 1);
  // stable sort: the table is a permutation of the input, ascending in zi, input order within a zi
  std::vector<int> order((size_t)n);
  for (int t = 0; t < n; ++t) order[(size_t)t] = t;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return (z[(size_t)a] & inner) < (z[(size_t)b] & inner); });
  for (int i = 0; i < n; ++i) {
    CHECK(d.terms[(size_t)i].zo == (z[(size_t)order[(size_t)i]] & ~inner));
    CHECK(std::memcmp(&d.terms[(size_t)i].c, &c[(size_t)order[(size_t)i]], sizeof(double)) == 0);
  }
}

// what k_diag_tile computes for the tile at `base`: E over the 2^11 slots (E(j) repeats above 2^tb)
static std::vector<double> tile_energies(const DiagTable& d, u64 base) {
  std::vector<double> W(1u << kExpTileBits, 0.0), slots((size_t)std::max(d.n_slots, 1), 0.0);
  for (const DiagPiece& pc : d.pieces) {
    double v = 0.0;
    for (int i = 0; i < pc.count; ++i) {
      const DiagTerm& t = d.terms[(size_t)(pc.first + i)];
      v += (__builtin_popcountll(base & t.zo) & 1) ? -t.c : t.c;
    }
    if (pc.slot < 0) W[pc.zi] = v;
    else slots[(size_t)pc.slot] = v;
  }
  for (const DiagJoin& j : d.joins) {
    double v = slots[(size_t)j.slot];
    for (int i = 1; i < j.count; ++i) v += slots[(size_t)(j.slot + i)];
    W[j.zi] = v;
  }
  for (int s = 0; s < kExpTileBits; ++s)
    for (size_t i = 0; i < W.size(); ++i)
      if (!((i >> s) & 1)) {
        const double p = W[i], q = W[i | (1u << s)];
        W[i] = p + q;
        W[i | (1u << s)] = p - q;
      }
  return W;
}

static void check_energies(int k, const std::vector<uint64_t>& z, const std::vector<double>& c, const DiagTable& d, double* worst) {
  const int tb = std::min(k, kExpTileBits), n = (int)z.size();
  double total = 0.0;
  for (double v : c) total += std::fabs(v);
  const u64 n_tiles = 1ull << (k - tb);
  for (u64 o = 0; o < n_tiles; o += std::max<u64>(1, n_tiles / 5)) {
    const u64 base = o << tb;
    const std::vector<double> E = tile_energies(d, base);
    for (u64 j = 0; j < (1ull << kExpTileBits); j += 37) {
      const u64 i = base | (j & ((1ull << tb) - 1));
      long double want = 0;
      for (int t = 0; t < n; ++t) want += (__builtin_popcountll(i & z[(size_t)t]) & 1) ? -c[(size_t)t] : c[(size_t)t];
      const double err = std::fabs((double)(E[j] - want)) / std::max(total, 1e-300);
      *worst = std::max(*worst, err);
    }
  }
}

// ---- the per-term values (qsim_expectation_z_terms): the records and passes of diag_value_table
static void check_value_table(int tb, int n, const std::vector<uint64_t>& z, const DiagValueTable& d) {
  const u64 inner = (1ull << tb) - 1;
  CHECK((int)d.terms.size() == n);
  for (int t = 0; t < n; ++t) {                     // input order, nothing merged: record t is term t
    const DiagValueTerm& r = d.terms[(size_t)t];
    CHECK(r.zi <= inner && (r.zo & inner) == 0 && ((u64)r.zi | r.zo) == z[(size_t)t] && r.pad_ == 0);
  }
  CHECK((int)d.passes.size() == (n + kDiagValuesPerPass - 1) / kDiagValuesPerPass);
  int next = 0;
  for (const DiagValuePass& p : d.passes) {
    CHECK(p.first == next && p.count >= 1 && p.count <= kDiagValuesPerPass);
    next += p.count;
  }
  CHECK(next == n);
  for (size_t i = 0; i + 1 < d.passes.size(); ++i) CHECK(d.passes[i].count == kDiagValuesPerPass);   // only the last one is short
}

// what k_diag_term_values and the row sum compute for one pass: per tile the unscaled transform of p = |psi|^2 (zero
// above 2^tb), a gather at zi with the outer sign, added over the tiles o = wg, wg + grid, ... of a "workgroup", then the
// rows in workgroup order
static std::vector<double> value_pass_model(int k, const std::vector<double>& p, const DiagValueTable& d, const DiagValuePass& ps, unsigned grid) {
  const int tb = std::min(k, kExpTileBits);
  const u64 n_tiles = 1ull << (k - tb);
  std::vector<std::vector<double>> rows(grid, std::vector<double>((size_t)ps.count, 0.0));
  std::vector<double> P(1u << kExpTileBits);
  for (unsigned wg = 0; wg < grid; ++wg)
    for (u64 o = wg; o < n_tiles; o += grid) {
      const u64 base = o << tb;
      for (size_t j = 0; j < P.size(); ++j) P[j] = j < (1ull << tb) ? p[(size_t)(base | j)] : 0.0;
      for (int s : {8, 9, 10, 0, 1, 2, 3, 4, 5, 6, 7})   // the kernel's order of the stages
        for (size_t i = 0; i < P.size(); ++i)
          if (!((i >> s) & 1)) {
            const double a = P[i], b = P[i | (1u << s)];
            P[i] = a + b;
            P[i | (1u << s)] = a - b;
          }
      for (int i = 0; i < ps.count; ++i) {
        const DiagValueTerm& r = d.terms[(size_t)(ps.first + i)];
        CHECK(r.zi < P.size());
        const double v = P[r.zi];
        rows[wg][(size_t)i] += (__builtin_popcountll(base & r.zo) & 1) ? -v : v;
      }
    }
  std::vector<double> out((size_t)ps.count, 0.0);
  for (unsigned wg = 0; wg < grid; ++wg)
    for (int i = 0; i < ps.count; ++i) out[(size_t)i] += rows[wg][(size_t)i];
  return out;
}

static void check_values(std::mt19937_64& rng, double* worst, int* cases) {
  struct Case { int k, n; int kind; unsigned grid; };   // kind 0: random masks, 1: inner part 0, 2: singles, pairs, identity and duplicates
  const Case list[] = {{1, 3, 0, 1024}, {5, 40, 0, 1024}, {10, 70, 2, 1024}, {11, 300, 0, 1024}, {12, 2047, 0, 1024}, {12, 2048, 0, 1024},
                       {12, 2049, 0, 1024}, {13, 120, 2, 3}, {14, 4100, 0, 5}, {16, 600, 2, 8}, {16, 64, 1, 7}, {12, 0, 0, 1024}};
  std::uniform_real_distribution<double> uni(0.0, 1.0);
  for (const Case& cs : list) {
    const int tb = std::min(cs.k, kExpTileBits);
    const u64 all = (1ull << cs.k) - 1, inner = (1ull << tb) - 1;
    std::vector<uint64_t> z;
    if (cs.kind == 2) {
      z.push_back(0);
      for (int a = 0; a < cs.k; ++a) z.push_back(1ull << a);
      for (int a = 0; a < cs.k; ++a)
        for (int b = a + 1; b < cs.k; ++b) z.push_back((1ull << a) | (1ull << b));
      z.push_back(all);
      z.push_back(z[3]);                            // duplicates: equal bits expected
      z.push_back(0);
      while ((int)z.size() < cs.n) z.push_back(rng() & all);
    } else {
      for (int t = 0; t < cs.n; ++t) z.push_back(cs.kind == 1 ? (rng() & all & ~inner) : (rng() & all));
    }
    const int n = (int)z.size();
    double out_stub = 0.0;
    CHECK(check_diag_args(cs.k, n, z.data(), &out_stub, false, nullptr, "check") == QSIM_OK);
    DiagValueTable d;
    diag_value_table(tb, n, z.data(), &d);
    check_value_table(tb, n, z, d);
    std::vector<double> p((size_t)1 << cs.k);
    double total = 0.0;
    for (double& v : p) { v = uni(rng); total += v; }
    for (double& v : p) v /= total;                 // weights of a unit-norm state
    const unsigned grid = (unsigned)std::min<u64>(1ull << (cs.k - tb), cs.grid);
    std::vector<double> got;
    for (const DiagValuePass& ps : d.passes) {
      const std::vector<double> part = value_pass_model(cs.k, p, d, ps, grid);
      got.insert(got.end(), part.begin(), part.end());
    }
    CHECK((int)got.size() == n);
    const int step = n > 400 ? 7 : 1;               // (a long list: every seventh term and both sides of every pass boundary)
    for (int t = 0; t < n && t < (int)got.size(); ++t) {
      if (t % step && (t % kDiagValuesPerPass) > 1 && (t % kDiagValuesPerPass) < kDiagValuesPerPass - 2) continue;
      long double want = 0;
      for (u64 i = 0; i <= all; ++i) want += (__builtin_popcountll(i & z[(size_t)t]) & 1) ? -(long double)p[(size_t)i] : (long double)p[(size_t)i];
      *worst = std::max(*worst, std::fabs((double)(got[(size_t)t] - want)));
    }
    if (cs.kind == 2) CHECK(std::memcmp(&got[3], &got[(size_t)(1 + cs.k + cs.k * (cs.k - 1) / 2 + 1)], sizeof(double)) == 0);
    ++*cases;
  }
}

int main() {
  std::mt19937_64 rng(12345);
  std::uniform_real_distribution<double> coef(-1.0, 1.0);
  double worst = 0.0;
  int cases = 0;
  struct Case { int k, n; int kind; };              // kind 0: random masks, 1: every inner part 0, 2: seven inner parts, 3: one mask
  const Case list[] = {{1, 1, 0}, {1, 5, 0}, {5, 40, 0}, {11, 300, 0}, {12, 0, 0}, {13, 64, 0}, {13, 65, 1}, {14, 2048, 0}, {14, 300, 2},
                       {16, 16384, 0}, {16, 16384, 1}, {16, 16384, 3}, {20, 129, 1}, {30, 435, 0}, {12, 4096, 2}, {63, 100, 0}};
  for (const Case& cs : list) {
    const int tb = std::min(cs.k, kExpTileBits);
    const u64 all = cs.k >= 64 ? ~0ull : (1ull << cs.k) - 1, inner = (1ull << tb) - 1;
    std::vector<uint64_t> z((size_t)cs.n);
    std::vector<double> c((size_t)cs.n);
    u64 seven[7];
    for (u64& s : seven) s = rng() & inner;
    for (int t = 0; t < cs.n; ++t) {
      u64 m = rng() & all;
      if (cs.kind == 1) m &= ~inner;
      if (cs.kind == 2) m = (m & ~inner) | seven[rng() % 7];
      if (cs.kind == 3) m = all;
      z[(size_t)t] = m;
      c[(size_t)t] = t % 11 == 3 ? 0.0 : coef(rng);
    }
    double gamma = 0.5;
    CHECK(check_diag_args(cs.k, cs.n, z.data(), c.data(), true, &gamma, "check") == QSIM_OK);
    DiagTable d;
    diag_table(tb, cs.n, z.data(), c.data(), &d);
    check_tables(tb, cs.n, z, c, d);
    if (cs.kind == 1 && cs.n > 0) CHECK((int)d.pieces.size() == (cs.n + kDiagPiece - 1) / kDiagPiece && d.joins.size() == (cs.n > kDiagPiece ? 1u : 0u));
    if (cs.k <= 30) check_energies(cs.k, z, c, d, &worst);
    ++cases;
  }
  std::printf("%d lists: tables consistent; host model of the tile against the direct sum: max |E - want| / sum|c| = %.3e\n", cases, worst);
  CHECK(worst < 1e-13);

  // the argument checks
  const uint64_t z2[2] = {1, 6};
  const double c2[2] = {0.1, 0.2};
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  double g = 0.3;
  CHECK(check_diag_args(14, 2, z2, c2, true, &g, "f") == QSIM_OK);
  CHECK(check_diag_args(14, 2, z2, c2, true, nullptr, "f") == QSIM_OK);
  CHECK(check_diag_args(14, 0, nullptr, nullptr, true, &g, "f") == QSIM_OK);
  CHECK(check_diag_args(14, -1, z2, c2, true, &g, "f") == QSIM_ERR_INVALID);
  CHECK(check_diag_args(14, kDiagMaxTerms + 1, z2, c2, true, &g, "f") == QSIM_ERR_INVALID);   // (refused before anything is read)
  CHECK(check_diag_args(14, 2, nullptr, c2, true, &g, "f") == QSIM_ERR_INVALID);
  CHECK(check_diag_args(14, 2, z2, nullptr, true, &g, "f") == QSIM_ERR_INVALID);
  for (double bad : {inf, -inf, nan}) {
    double gb = bad;
    const double cb[2] = {0.1, bad};
    CHECK(check_diag_args(14, 2, z2, c2, true, &gb, "f") == QSIM_ERR_INVALID);
    CHECK(check_diag_args(14, 2, z2, cb, true, &g, "f") == QSIM_ERR_INVALID);
  }
  for (u64 bad : {1ull << 14, 1ull << 15, 1ull << 63}) {
    const uint64_t zb[2] = {1, bad};
    CHECK(check_diag_args(14, 2, zb, c2, true, &g, "f") == QSIM_ERR_NONLOCAL);
    CHECK(g_err.find("term 1 acts on index bit") != std::string::npos && g_err.find("log2(chunk_size)=14") != std::string::npos);
  }
  const uint64_t top[1] = {1ull << 63};
  CHECK(check_diag_args(64, 1, top, c2, true, &g, "f") == QSIM_OK);

  // the per-term values: tables, the host model of the pass against the direct sum, the argument checks
  double worst_value = 0.0;
  int value_cases = 0;
  check_values(rng, &worst_value, &value_cases);
  std::printf("%d lists of single terms: records and passes consistent; host model of the pass against the direct sum: max |value - want| = %.3e\n",
              value_cases, worst_value);
  CHECK(worst_value < 1e-12);                       // the bound of the device tests, on weights of total 1
  double o2[2] = {0.0, 0.0};
  CHECK(check_diag_args(14, 2, z2, o2, false, nullptr, "f") == QSIM_OK);
  CHECK(check_diag_args(14, 0, nullptr, nullptr, false, nullptr, "f") == QSIM_OK);
  CHECK(check_diag_args(14, -1, z2, o2, false, nullptr, "f") == QSIM_ERR_INVALID && g_err == "f: n_terms = -1");
  CHECK(check_diag_args(14, kDiagMaxTerms + 1, z2, o2, false, nullptr, "f") == QSIM_ERR_INVALID);   // (refused before anything is read)
  CHECK(g_err.find("16385 terms in one call, at most 16384") != std::string::npos);
  CHECK(check_diag_args(14, 2, nullptr, o2, false, nullptr, "f") == QSIM_ERR_INVALID && g_err == "f: null argument");
  CHECK(check_diag_args(14, 2, z2, nullptr, false, nullptr, "f") == QSIM_ERR_INVALID && g_err == "f: null argument");
  CHECK(check_diag_args(14, -1, nullptr, nullptr, false, nullptr, "f") == QSIM_ERR_INVALID && g_err == "f: n_terms = -1");   // n_terms before null
  for (u64 bad : {1ull << 14, 1ull << 15, 1ull << 63}) {
    const uint64_t zb[2] = {1, bad};
    CHECK(check_diag_args(14, 2, zb, o2, false, nullptr, "f") == QSIM_ERR_NONLOCAL);
    CHECK(g_err.find("term 1 acts on index bit") != std::string::npos && g_err.find("log2(chunk_size)=14") != std::string::npos);
  }
  CHECK(check_diag_args(64, 1, top, o2, false, nullptr, "f") == QSIM_OK);
  if (g_failed) { std::printf("diag_plan_check: %d checks FAILED\n", g_failed); return 1; }
  std::printf("diag_plan_check: ok\n");
  return 0;
}
