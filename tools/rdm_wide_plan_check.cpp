// Stand-alone host check of quantum_simulations_amd/csrc/rdm_wide_plan.h: the plan of qsim_reduced_density_matrix_wide
// (roles of the qubits, tile, masks, pairs, slices, workspace, index map) for every r = 7..12 at k = r .. r + 6 and at
// k = 22, 28, 30, 32 under the placements of tests/test_gpu_density_wide.py; a host restatement of the whole pass --
// the same blocks, pairs, slices, staging order, partial blocks, row sum and assembly as k_rdm_wide, plain loops in
// place of the MFMAs -- against the direct definition at small k; every argument refusal.  No GPU, no HIP.  Meant for
// the host sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/rdm_wide_plan_check.cpp -o rdm_wide_plan_check && ./rdm_wide_plan_check
// Exit status 0 and a last line "rdm_wide_plan_check: ok" mean that every case passed.
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

#include "../quantum_simulations_amd/csrc/rdm_wide_plan.h"

static int g_failed = 0;
#define CHECK(cond)                                                              \
  do {                                                                           \
    if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_failed; } \
  } while (0)

typedef std::vector<int32_t> Qubits;

// the placements of the device tests on a chunk of k bits (those that fit), each ascending, descending and shuffled
static std::vector<Qubits> placements(int k, int r, std::mt19937_64& rng) {
  std::vector<Qubits> base;
  Qubits q;
  for (int i = 0; i < r; ++i) q.push_back(i);                       // all three line bits
  base.push_back(q);
  q.clear();
  for (int i = 0; i < r; ++i) q.push_back(k - r + i);               // the top r
  base.push_back(q);
  if (r + 3 <= k) {                                                  // no line bit
    q.clear();
    for (int i = 0; i < r; ++i) q.push_back(3 + i);
    base.push_back(q);
  }
  if (k >= r + 4) {                                                  // spread with exactly one line bit
    q.assign(1, 1);
    for (int i = 0; i < r - 1; ++i) q.push_back((int32_t)std::lround(4 + (double)i * (k - 1 - 4) / (r - 2)));
    base.push_back(q);
  }
  {                                                                  // a random subset
    Qubits all;
    for (int i = 0; i < k; ++i) all.push_back(i);
    std::shuffle(all.begin(), all.end(), rng);
    all.resize((size_t)r);
    base.push_back(all);
  }
  std::vector<Qubits> out;
  for (Qubits b : base) {
    std::sort(b.begin(), b.end());
    out.push_back(b);
    Qubits d(b.rbegin(), b.rend());                                  // the block qubits first in the caller's list
    out.push_back(d);
    std::shuffle(b.begin(), b.end(), rng);
    out.push_back(b);
  }
  return out;
}

static void check_plan(int k, int r, const Qubits& qs, int max_wg) {
  RdmWidePlan p;
  rdm_wide_plan(k, r, qs.data(), &p, max_wg);
  const u64 all = k >= 64 ? ~0ull : (1ull << k) - 1;
  u64 sel = 0;
  for (int q : qs) sel |= 1ull << q;
  CHECK(p.k == k && p.r == r && p.nb_bits == r - 6 && p.nb == 1 << (r - 6));
  CHECK(p.tb == std::min(11, k - (r - 6)) && p.eb == p.tb - 6 && p.eb >= 0);
  CHECK((p.tile_mask & p.block_mask) == 0 && (p.tile_mask & p.outer_mask) == 0 && (p.block_mask & p.outer_mask) == 0);
  CHECK((p.tile_mask | p.block_mask | p.outer_mask) == all);
  CHECK(__builtin_popcountll(p.tile_mask) == p.tb && __builtin_popcountll(p.block_mask) == r - 6);
  CHECK((p.outer_mask & sel) == 0 && (p.block_mask & ~sel) == 0);
  CHECK((p.tile_mask & 7ull) == (all & 7ull));                       // whole lines
  CHECK(p.n_outer == 1ull << __builtin_popcountll(p.outer_mask));
  u64 rows = 0;
  for (int q = 0; q < 6; ++q) {
    CHECK(p.row_phys[q] >= 0 && p.row_phys[q] < k && ((sel >> p.row_phys[q]) & 1));
    CHECK(qs[(size_t)p.row_pos[q]] == p.row_phys[q]);
    if (q) CHECK(p.row_phys[q] > p.row_phys[q - 1]);
    rows |= 1ull << p.row_phys[q];
  }
  CHECK((rows & ~p.tile_mask) == 0 && (rows | p.block_mask) == sel);
  CHECK((sel & 7ull & ~rows) == 0);                                  // a selected line bit is a row qubit
  for (int b = 0; b < r - 6; ++b) {
    CHECK(qs[(size_t)p.blk_pos[b]] == p.blk_phys[b] && ((p.block_mask >> p.blk_phys[b]) & 1));
    CHECK(p.blk_phys[b] > p.row_phys[5]);                            // the rows are the lowest selected bits
    if (b) CHECK(p.blk_phys[b] > p.blk_phys[b - 1]);
  }
  // the e' bits are the LOWEST free bits: no free bit below the highest e' bit is left out of the tile
  const u64 env = p.tile_mask & ~sel;
  if (env) {
    const int top = 63 - __builtin_clzll(env);
    CHECK((((1ull << top) - 1) & ~sel & ~p.tile_mask) == 0);
  }
  u64 seen_phys = 0;
  unsigned seen_lds = 0;
  for (int t = 0; t < p.tb; ++t) {
    CHECK((p.tile_mask >> p.phys_bit[t]) & 1);
    if (t) CHECK(p.phys_bit[t] > p.phys_bit[t - 1]);
    CHECK(p.lds_pos[t] >= 0 && p.lds_pos[t] < p.tb);
    seen_phys |= 1ull << p.phys_bit[t];
    seen_lds |= 1u << p.lds_pos[t];
    const bool is_row = (rows >> p.phys_bit[t]) & 1;
    CHECK(is_row == (p.lds_pos[t] >= p.eb));
    if (is_row) CHECK(p.row_phys[p.lds_pos[t] - p.eb] == p.phys_bit[t]);
  }
  CHECK(seen_phys == p.tile_mask && seen_lds == (1u << p.tb) - 1);
  CHECK(p.pairs == p.nb * (p.nb + 1) / 2);
  CHECK(p.slices >= 1 && (p.slices & (p.slices - 1)) == 0 && (u64)p.slices <= p.n_outer);
  CHECK(p.grid == (unsigned)p.pairs * p.slices && (int)p.grid <= std::max(max_wg, p.pairs));
  if ((u64)(2 * p.slices) <= p.n_outer) CHECK((u64)p.pairs * 2 * p.slices > (u64)max_wg);   // S is the largest allowed
  CHECK(p.work_bytes == 65536ull * ((u64)p.grid + (p.slices > 1 ? (u64)p.pairs : 0)));
  for (int pr = 0, I = 0; I < p.nb; ++I)
    for (int J = 0; J <= I; ++J, ++pr) CHECK(rdm_tile_row(pr) == I && rdm_tile_col(pr) == J);
  // deposit and index map: the amplitude (block pattern I, row pattern a) has the caller's index rdm_wide_index(I, a)
  std::vector<char> hit((size_t)1 << r, 0);
  for (int I = 0; I < p.nb; ++I) {
    const u64 d = rdm_wide_deposit(p, I);
    CHECK((d & ~p.block_mask) == 0 && __builtin_popcountll(d) == __builtin_popcount((unsigned)I));
    for (int a = 0; a < 64; ++a) {
      u64 i = d;
      for (int q = 0; q < 6; ++q) i |= (u64)((a >> q) & 1) << p.row_phys[q];
      int want = 0;
      for (int j = 0; j < r; ++j) want |= (int)((i >> qs[(size_t)j]) & 1) << j;
      const int x = rdm_wide_index(p, I, a);
      CHECK(x == want && x >= 0 && x < (1 << r));
      if (x >= 0 && x < (1 << r)) ++hit[(size_t)x];
    }
  }
  for (char h : hit) CHECK(h == 1);
}

static u64 deposit(u64 mask, u64 o) {               // tile_base of the device
  u64 base = 0;
  while (mask) {
    const u64 low = mask & (~mask + 1);
    if (o & 1) base |= low;
    o >>= 1;
    mask ^= low;
  }
  return base;
}

// the pass as the device runs it, against the definition; returns the largest deviation
static double model_pass(int k, int r, const Qubits& qs, int max_wg, std::mt19937_64& rng) {
  typedef std::complex<double> cd;
  RdmWidePlan p;
  rdm_wide_plan(k, r, qs.data(), &p, max_wg);
  const u64 n = 1ull << k;
  std::vector<cd> psi((size_t)n);
  std::normal_distribution<double> gauss;
  double norm = 0;
  for (cd& v : psi) { v = cd(gauss(rng), gauss(rng)); norm += std::norm(v); }
  for (cd& v : psi) v /= std::sqrt(norm);
  const int E = 1 << p.eb, S = 1 << p.tb;
  std::vector<double> partial((size_t)p.grid * kRdmWideBlockDoubles, std::nan(""));   // what no workgroup writes must not be read
  std::vector<cd> ti((size_t)64 * E), tj((size_t)64 * E);
  const auto stage = [&](u64 base, std::vector<cd>& tile) {
    for (int j = 0; j < S; ++j) {
      u64 o = 0;
      int l = 0;
      for (int b = 0; b < p.tb; ++b) { o |= (u64)((j >> b) & 1) << p.phys_bit[b]; l |= ((j >> b) & 1) << p.lds_pos[b]; }
      CHECK((base | o) < n);
      tile[(size_t)l] = psi[(size_t)(base | o)];
    }
  };
  for (unsigned wg = 0; wg < p.grid; ++wg) {
    const int pair = (int)(wg % (unsigned)p.pairs);
    const u64 slice = wg / (unsigned)p.pairs;
    const int I = rdm_tile_row(pair), J = rdm_tile_col(pair);
    std::vector<cd> acc(4096, cd(0, 0));
    for (u64 o = slice; o < p.n_outer; o += p.slices) {
      const u64 base = deposit(p.outer_mask, o);
      stage(base | rdm_wide_deposit(p, I), ti);
      if (J != I) stage(base | rdm_wide_deposit(p, J), tj);
      const std::vector<cd>& tjj = J != I ? tj : ti;
      for (int a = 0; a < 64; ++a)
        for (int b = 0; b < 64; ++b) {
          if (I == J && (b >> 4) > (a >> 4)) continue;   // the 16 x 16 tiles of the lower triangle
          for (int e = 0; e < E; ++e) acc[(size_t)(a * 64 + b)] += ti[(size_t)((a << p.eb) | e)] * std::conj(tjj[(size_t)((b << p.eb) | e)]);
        }
    }
    double* mine = partial.data() + ((size_t)slice * p.pairs + pair) * kRdmWideBlockDoubles;
    for (int a = 0; a < 64; ++a)
      for (int b = 0; b < 64; ++b) {
        if (I == J && (b >> 4) > (a >> 4)) continue;
        mine[a * 64 + b] = acc[(size_t)(a * 64 + b)].real();
        mine[4096 + a * 64 + b] = acc[(size_t)(a * 64 + b)].imag();
      }
  }
  const size_t cols = (size_t)p.pairs * kRdmWideBlockDoubles;
  std::vector<double> blocks(cols);
  for (size_t c = 0; c < cols; ++c) {                // k_hist_sum: the rows in row order
    double v = 0.0;
    for (unsigned s = 0; s < p.slices; ++s) v += partial[(size_t)s * cols + c];
    blocks[c] = v;
  }
  const u64 dim = 1ull << r;
  std::vector<double> out((size_t)(2 * dim * dim), std::nan(""));
  rdm_wide_assemble(p, blocks.data(), out.data());
  // the definition: rho[x][y] = sum over e of psi(e, x) conj(psi(e, y))
  u64 sel = 0;
  for (int q : qs) sel |= 1ull << q;
  std::vector<u64> spread((size_t)dim);
  for (u64 x = 0; x < dim; ++x) {
    u64 i = 0;
    for (int j = 0; j < r; ++j) i |= ((x >> j) & 1) << qs[(size_t)j];
    spread[(size_t)x] = i;
  }
  std::vector<cd> rho((size_t)(dim * dim), cd(0, 0));
  for (u64 e = 0; e < n; ++e) {
    if (e & sel) continue;
    for (u64 x = 0; x < dim; ++x) {
      const cd vx = psi[(size_t)(e | spread[(size_t)x])];
      for (u64 y = 0; y < dim; ++y) rho[(size_t)(x * dim + y)] += vx * std::conj(psi[(size_t)(e | spread[(size_t)y])]);
    }
  }
  double worst = 0;
  for (u64 x = 0; x < dim; ++x) {
    CHECK(out[(size_t)(2 * (x * dim + x) + 1)] == 0.0);
    for (u64 y = 0; y < dim; ++y) {
      const double re = out[(size_t)(2 * (x * dim + y))], im = out[(size_t)(2 * (x * dim + y) + 1)];
      CHECK(re == out[(size_t)(2 * (y * dim + x))] && im == -out[(size_t)(2 * (y * dim + x) + 1)]);   // exactly Hermitian
      const double d = std::abs(cd(re, im) - rho[(size_t)(x * dim + y)]);
      if (!(d <= worst)) worst = d;                  // (a NaN shows)
    }
  }
  return worst;
}

static void check_refusals() {
  const char* what = "qsim_reduced_density_matrix_wide";
  int32_t q[13] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12};
  double out[1];
  CHECK(rdm_wide_check_count(7, nullptr, out, what) == QSIM_ERR_INVALID && g_err.find("null argument") != std::string::npos);
  CHECK(rdm_wide_check_count(7, q, nullptr, what) == QSIM_ERR_INVALID && g_err.find("null argument") != std::string::npos);
  for (int r : {-1, 0, 1, 6, 13, 64}) {
    CHECK(rdm_wide_check_count(r, q, out, what) == QSIM_ERR_INVALID);
    CHECK(g_err.find("7 <= r <= 12") != std::string::npos && g_err.find("qsim_reduced_density_matrix serves r <= 6") != std::string::npos);
  }
  for (int r = 7; r <= 12; ++r) {
    CHECK(rdm_wide_check_count(r, q, out, what) == QSIM_OK);
    CHECK(rdm_wide_check_qubits(r, r, q, what) == QSIM_OK);
    CHECK(rdm_wide_check_qubits(r - 1, r, q, what) == QSIM_ERR_NONLOCAL);
    CHECK(g_err == "qubit " + std::to_string(r - 1) + " >= log2(chunk_size)=" + std::to_string(r - 1) + ": non-local gate requires layout/collect step");
    int32_t rep[12];
    std::copy(q, q + 12, rep);
    rep[r - 1] = rep[2];
    CHECK(rdm_wide_check_qubits(14, r, rep, what) == QSIM_ERR_INVALID && g_err == std::string(what) + ": repeated qubit 2");
    rep[r - 1] = -3;
    CHECK(rdm_wide_check_qubits(14, r, rep, what) == QSIM_ERR_INVALID && g_err == "qubit -3 is negative");
  }
}

int main() {
  std::mt19937_64 rng(30);
  int plans = 0;
  for (int r = 7; r <= 12; ++r) {
    std::vector<int> ks;
    for (int k = r; k <= r + 6; ++k) ks.push_back(k);
    for (int k : {22, 28, 30, 32}) ks.push_back(k);
    for (int k : ks)
      for (const Qubits& qs : placements(k, r, rng))
        for (int max_wg : {kRdmWideMaxWg, 4, 64}) { check_plan(k, r, qs, max_wg); ++plans; }
  }
  std::printf("plans checked: %d\n", plans);
  // the documented workspace at full size (30 qubits)
  {
    const double want_mib[6] = {96.1875, 80.625, 74.25, 76.5, 99.0, 130.0};
    for (int r = 7; r <= 12; ++r) {
      Qubits qs;
      for (int i = 0; i < r; ++i) qs.push_back(2 * i + 1);
      RdmWidePlan p;
      rdm_wide_plan(30, r, qs.data(), &p);
      CHECK((double)p.work_bytes / 1048576.0 == want_mib[r - 7]);
      std::printf("r=%d at 30 qubits: pairs %d, slices %u, grid %u, workspace %.3f MiB\n", r, p.pairs, p.slices, p.grid, (double)p.work_bytes / 1048576.0);
    }
  }
  // the host model: chunks smaller than a tile (k = r, r + 1, r + 2), the first full tile, several outer tiles per slice
  double worst = 0;
  for (int r = 7; r <= 12; ++r) {
    for (int k = r; k <= 14; ++k) {
      if (r >= 11 && k > r + 1) break;               // 4^r x 2^(k - r) complex products each: keep the run short
      if (r >= 9 && k > r + 3) break;
      const std::vector<Qubits> sets = placements(k, r, rng);
      for (size_t i = 0; i < sets.size(); i += (r >= 10 ? 4 : 1))
        for (int max_wg : {kRdmWideMaxWg, 4}) {
          if (r >= 10 && max_wg == 4 && i) continue;
          const double d = model_pass(k, r, sets[i], max_wg, rng);
          CHECK(d < 1e-14);
          worst = std::max(worst, d);
        }
    }
  }
  // r = 10 with the first full tile (k = 15: E = 32, 136 pairs), one spread set
  {
    const Qubits qs = {1, 4, 5, 7, 8, 10, 11, 12, 13, 14};
    RdmWidePlan p;
    rdm_wide_plan(15, 10, qs.data(), &p);
    CHECK(p.tb == 11 && p.pairs == 136);
    const double d = model_pass(15, 10, qs, kRdmWideMaxWg, rng);
    CHECK(d < 1e-14);
    worst = std::max(worst, d);
  }
  // r = 7 and 8 with a workgroup that walks several outer tiles: the cap lowered so that n_outer > S
  for (int r : {7, 8})
    for (int k : {r + 7, r + 8}) {
      Qubits qs = {2, 9, 0, (int32_t)(k - 1), 12, 5, 7};
      if (r == 8) qs.push_back(10);
      RdmWidePlan p;
      rdm_wide_plan(k, r, qs.data(), &p, 8);
      CHECK(p.n_outer / p.slices >= 2);
      const double d = model_pass(k, r, qs, 8, rng);
      CHECK(d < 1e-14);
      worst = std::max(worst, d);
    }
  std::printf("host model: max |model - definition| = %.3e (bound 1e-14)\n", worst);
  check_refusals();
  if (g_failed) { std::printf("rdm_wide_plan_check: %d FAILED\n", g_failed); return 1; }
  std::printf("rdm_wide_plan_check: ok\n");
  return 0;
}
