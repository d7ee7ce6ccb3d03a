// Stand-alone host check of quantum_simulations_amd/csrc/rdm_plan.h, the host side of both reduced-density-matrix calls.
// qsim_reduced_density_matrix_wide: the plan (roles of the qubits, tile, masks, pairs, slices, workspace, index map) for
// every r = 7..12 at k = r .. r + 6 and at k = 22, 28, 30, 32 under the placements of tests/test_gpu_density_wide.py; a
// host restatement of the whole pass -- the same blocks, pairs, slices, staging order, partial blocks, row sum and
// assembly as k_rdm_wide, plain loops in place of the MFMAs -- against the direct definition at small k.
// qsim_reduced_density_matrix: the plan (tile, masks, swizzle, grid, workspace) for every r = 1..6 at k = r .. r + 6, 14,
// 22, 23, 30 under the same placements and orders; the pass -- staging by LDS index with the swizzle of r <= 3 and the
// padded rows of r >= 4, a partial triangle per workgroup, row sum, mirror -- against the definition at small k.
// No GPU, no HIP.  Meant for the host sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/rdm_plan_check.cpp -o rdm_plan_check && ./rdm_plan_check
// Exit status 0 and a last line "rdm_plan_check: ok" mean that every case passed.
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

typedef unsigned long long u64;

#include "../quantum_simulations_amd/csrc/rdm_plan.h"

static int g_failed = 0;
#define CHECK(cond)                                                              \
  do {                                                                           \
    if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_failed; } \
  } while (0)

typedef std::vector<int32_t> Qubits;
typedef std::complex<double> cd;

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
    for (int i = 0; i < r - 1; ++i) q.push_back(r == 2 ? k - 1 : (int32_t)std::lround(4 + (double)i * (k - 1 - 4) / (r - 2)));
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

static u64 mask_of(const Qubits& qs) {
  u64 sel = 0;
  for (int q : qs) sel |= 1ull << q;
  return sel;
}

// what both plans ask of a tile: rows[q] is row bit q; the selected bits outside the rows are `blocks`
static void check_layout(int k, const RdmTileLayout& t, u64 sel, const int* rows, int n_rows, u64 blocks) {
  const u64 all = k >= 64 ? ~0ull : (1ull << k) - 1;
  CHECK(t.eb == t.tb - n_rows && t.eb >= 0 && t.tb <= kRdmTileBits);
  CHECK((t.tile_mask & blocks) == 0 && (t.tile_mask & t.outer_mask) == 0 && (blocks & t.outer_mask) == 0);
  CHECK((t.tile_mask | blocks | t.outer_mask) == all);
  CHECK(__builtin_popcountll(t.tile_mask) == t.tb);
  CHECK((t.outer_mask & sel) == 0);
  CHECK((t.tile_mask & 7ull) == (all & 7ull));                       // whole lines
  CHECK(t.n_tiles == 1ull << __builtin_popcountll(t.outer_mask));
  u64 row_mask = 0;
  for (int q = 0; q < n_rows; ++q) row_mask |= 1ull << rows[q];
  CHECK((row_mask & ~t.tile_mask) == 0 && (row_mask | blocks) == sel);
  // the e' bits are the LOWEST free bits: no free bit below the highest e' bit is left out of the tile
  const u64 env = t.tile_mask & ~sel;
  if (env) {
    const int top = 63 - __builtin_clzll(env);
    CHECK((((1ull << top) - 1) & ~sel & ~t.tile_mask) == 0);
  }
  u64 seen_phys = 0;
  unsigned seen_lds = 0;
  int last_env = -1;
  for (int b = 0; b < t.tb; ++b) {
    CHECK((t.tile_mask >> t.phys_bit[b]) & 1);
    if (b) CHECK(t.phys_bit[b] > t.phys_bit[b - 1]);
    CHECK(t.lds_pos[b] >= 0 && t.lds_pos[b] < t.tb);
    seen_phys |= 1ull << t.phys_bit[b];
    seen_lds |= 1u << t.lds_pos[b];
    const bool is_row = (row_mask >> t.phys_bit[b]) & 1;
    CHECK(is_row == (t.lds_pos[b] >= t.eb));
    if (is_row) CHECK(rows[t.lds_pos[b] - t.eb] == t.phys_bit[b]);  // row bit q at eb + q
    else { CHECK(t.lds_pos[b] == last_env + 1); last_env = t.lds_pos[b]; }   // e' bits ascending
  }
  CHECK(seen_phys == t.tile_mask && seen_lds == (1u << t.tb) - 1);
}

static void check_plan(int k, int r, const Qubits& qs, int max_wg) {
  RdmWidePlan p;
  rdm_wide_plan(k, r, qs.data(), &p, max_wg);
  const u64 sel = mask_of(qs);
  CHECK(p.k == k && p.r == r && p.nb_bits == r - 6 && p.nb == 1 << (r - 6));
  CHECK(p.t.tb == std::min(11, k - (r - 6)) && p.t.eb == p.t.tb - 6);
  CHECK(__builtin_popcountll(p.block_mask) == r - 6 && (p.block_mask & ~sel) == 0);
  check_layout(k, p.t, sel, p.row_phys, 6, p.block_mask);
  u64 rows = 0;
  for (int q = 0; q < 6; ++q) {
    CHECK(p.row_phys[q] >= 0 && p.row_phys[q] < k && ((sel >> p.row_phys[q]) & 1));
    CHECK(qs[(size_t)p.row_pos[q]] == p.row_phys[q]);
    if (q) CHECK(p.row_phys[q] > p.row_phys[q - 1]);
    rows |= 1ull << p.row_phys[q];
  }
  CHECK((sel & 7ull & ~rows) == 0);                                  // a selected line bit is a row qubit
  for (int b = 0; b < r - 6; ++b) {
    CHECK(qs[(size_t)p.blk_pos[b]] == p.blk_phys[b] && ((p.block_mask >> p.blk_phys[b]) & 1));
    CHECK(p.blk_phys[b] > p.row_phys[5]);                            // the rows are the lowest selected bits
    if (b) CHECK(p.blk_phys[b] > p.blk_phys[b - 1]);
  }
  CHECK(p.pairs == p.nb * (p.nb + 1) / 2);
  CHECK(p.slices >= 1 && (p.slices & (p.slices - 1)) == 0 && (u64)p.slices <= p.t.n_tiles);
  CHECK(p.grid == (unsigned)p.pairs * p.slices && (int)p.grid <= std::max(max_wg, p.pairs));
  if ((u64)(2 * p.slices) <= p.t.n_tiles) CHECK((u64)p.pairs * 2 * p.slices > (u64)max_wg);   // S is the largest allowed
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

static void check_narrow_plan(int k, int r, const Qubits& qs, int max_wg) {
  RdmPlan p;
  rdm_plan(k, r, qs.data(), &p, max_wg);
  const u64 sel = mask_of(qs);
  CHECK(p.r == r && p.t.tb == std::min(k, 11) && p.t.eb == p.t.tb - r);
  std::vector<int> rows(qs.begin(), qs.end());                       // the caller's order
  check_layout(k, p.t, sel, rows.data(), r, 0);
  CHECK(p.t.n_tiles == 1ull << (k - p.t.tb));
  // the swizzle: e' bits 0 .. n_free - 1 are the line bits outside the qubits; a qubit on a line bit takes one of the
  // e' bits from there up to bit 2, each one once
  const int n_free = __builtin_popcountll(~sel & ((1ull << std::min(k, 3)) - 1));
  unsigned taken = 0;
  for (int q = 0; q < 6; ++q) {
    const int s = p.swz[q];
    if (!s) continue;
    CHECK(q < r && qs[(size_t)q] < 3);
    CHECK((s & (s - 1)) == 0 && s >= (1 << n_free) && s < (1 << std::min(p.t.eb, 3)) && !(taken & (unsigned)s));
    taken |= (unsigned)s;
  }
  // ... and no such e' bit is left while a qubit on a line bit goes without
  int want = 0;
  for (int q : qs) want += q < 3;
  CHECK(__builtin_popcount(taken) == std::min(want, std::max(0, std::min(p.t.eb, 3) - n_free)));
  CHECK((u64)p.grid == std::min<u64>(p.t.n_tiles, (u64)max_wg));
  CHECK(p.work_bytes == 8ull * ((u64)p.grid + 1) * (1ull << (2 * r)));
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

static std::vector<cd> random_state(int k, std::mt19937_64& rng) {
  std::vector<cd> psi((size_t)1 << k);
  std::normal_distribution<double> gauss;
  double norm = 0;
  for (cd& v : psi) { v = cd(gauss(rng), gauss(rng)); norm += std::norm(v); }
  for (cd& v : psi) v /= std::sqrt(norm);
  return psi;
}

// rdm_thread_slots and rdm_fill of the device: the tile at `base` into LDS; lidx(l) is what the kernel makes of the LDS index
template <class Lidx>
static void stage(const RdmTileLayout& t, const std::vector<cd>& psi, u64 base, std::vector<cd>& tile, Lidx lidx) {
  for (int j = 0; j < (1 << t.tb); ++j) {
    u64 o = 0;
    int l = 0;
    for (int b = 0; b < t.tb; ++b) { o |= (u64)((j >> b) & 1) << t.phys_bit[b]; l |= ((j >> b) & 1) << t.lds_pos[b]; }
    CHECK((base | o) < psi.size());
    tile.at((size_t)lidx(l)) = psi[(size_t)(base | o)];
  }
}

// out (2 * 4^r doubles) against the definition rho[x][y] = sum over e of psi(e, x) conj(psi(e, y)): the largest
// deviation; out must be exactly Hermitian
static double deviation(int k, int r, const Qubits& qs, const std::vector<cd>& psi, const std::vector<double>& out) {
  const u64 n = 1ull << k, dim = 1ull << r, sel = mask_of(qs);
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

static std::vector<double> sum_rows(const std::vector<double>& partial, unsigned rows, size_t cols) {   // k_hist_sum: the rows in row order
  std::vector<double> sum(cols);
  for (size_t c = 0; c < cols; ++c) {
    double v = 0.0;
    for (unsigned s = 0; s < rows; ++s) v += partial[(size_t)s * cols + c];
    sum[c] = v;
  }
  return sum;
}

// the wide pass as the device runs it, against the definition; returns the largest deviation
static double model_pass(int k, int r, const Qubits& qs, int max_wg, std::mt19937_64& rng) {
  RdmWidePlan p;
  rdm_wide_plan(k, r, qs.data(), &p, max_wg);
  const std::vector<cd> psi = random_state(k, rng);
  const int E = 1 << p.t.eb;
  std::vector<double> partial((size_t)p.grid * kRdmWideBlockDoubles, std::nan(""));   // what no workgroup writes must not be read
  std::vector<cd> ti((size_t)64 * E), tj((size_t)64 * E);
  const auto plain = [](int l) { return l; };
  for (unsigned wg = 0; wg < p.grid; ++wg) {
    const int pair = (int)(wg % (unsigned)p.pairs);
    const u64 slice = wg / (unsigned)p.pairs;
    const int I = rdm_tile_row(pair), J = rdm_tile_col(pair);
    std::vector<cd> acc(4096, cd(0, 0));
    for (u64 o = slice; o < p.t.n_tiles; o += p.slices) {
      const u64 base = deposit(p.t.outer_mask, o);
      stage(p.t, psi, base | rdm_wide_deposit(p, I), ti, plain);
      if (J != I) stage(p.t, psi, base | rdm_wide_deposit(p, J), tj, plain);
      const std::vector<cd>& tjj = J != I ? tj : ti;
      for (int a = 0; a < 64; ++a)
        for (int b = 0; b < 64; ++b) {
          if (I == J && (b >> 4) > (a >> 4)) continue;   // the 16 x 16 tiles of the lower triangle
          for (int e = 0; e < E; ++e) acc[(size_t)(a * 64 + b)] += ti[(size_t)((a << p.t.eb) | e)] * std::conj(tjj[(size_t)((b << p.t.eb) | e)]);
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
  const std::vector<double> blocks = sum_rows(partial, p.slices, (size_t)p.pairs * kRdmWideBlockDoubles);
  std::vector<double> out((size_t)2 << (2 * r), std::nan(""));
  rdm_wide_assemble(p, blocks.data(), out.data());
  return deviation(k, r, qs, psi, out);
}

// the pass of r <= 6 as the device runs it: rows stored with e' ^ g(a) for r <= 3 (k_rdm_small), with stride E + 1 for
// r >= 4 (k_rdm_mfma), and read back the same way
static double model_narrow_pass(int k, int r, const Qubits& qs, int max_wg, std::mt19937_64& rng) {
  RdmPlan p;
  rdm_plan(k, r, qs.data(), &p, max_wg);
  const std::vector<cd> psi = random_state(k, rng);
  const int eb = p.t.eb, E = 1 << eb, D = 1 << r;
  const bool small = r <= 3;
  const auto g = [&](int a) {
    int x = 0;
    for (int q = 0; q < r; ++q) x ^= ((a >> q) & 1) ? p.swz[q] : 0;
    return x;
  };
  const auto lidx = [&](int l) { return small ? l ^ g(l >> eb) : l + (l >> eb); };
  const auto word = [&](int a, int e) { return small ? (a << eb) | (e ^ g(a)) : a * (E + 1) + e; };
  const cd hole(std::nan(""), std::nan(""));         // a word that staging leaves out must not be read
  std::vector<cd> tile((size_t)D * (E + 1));
  std::vector<double> partial((size_t)p.grid * D * D, std::nan(""));
  for (unsigned wg = 0; wg < p.grid; ++wg) {
    std::vector<cd> acc((size_t)D * D, cd(0, 0));
    for (u64 o = wg; o < p.t.n_tiles; o += p.grid) {
      std::fill(tile.begin(), tile.end(), hole);
      stage(p.t, psi, deposit(p.t.outer_mask, o), tile, lidx);
      for (int a = 0; a < D; ++a)
        for (int b = 0; b <= a; ++b)
          for (int e = 0; e < E; ++e) acc[(size_t)(a * D + b)] += tile[(size_t)word(a, e)] * std::conj(tile[(size_t)word(b, e)]);
    }
    double* mine = partial.data() + (size_t)wg * D * D;
    for (int a = 0; a < D; ++a)
      for (int b = 0; b <= a; ++b) {
        mine[a * D + b] = acc[(size_t)(a * D + b)].real();
        if (a > b) mine[b * D + a] = acc[(size_t)(a * D + b)].imag();
      }
  }
  const std::vector<double> tri = sum_rows(partial, p.grid, (size_t)D * D);
  std::vector<double> out((size_t)2 * D * D, std::nan(""));
  rdm_mirror(r, tri.data(), out.data());
  return deviation(k, r, qs, psi, out);
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
    CHECK(p.t.tb == 11 && p.pairs == 136);
    const double d = model_pass(15, 10, qs, kRdmWideMaxWg, rng);
    CHECK(d < 1e-14);
    worst = std::max(worst, d);
  }
  // r = 7 and 8 with a workgroup that walks several outer tiles: the cap lowered so that n_tiles > S
  for (int r : {7, 8})
    for (int k : {r + 7, r + 8}) {
      Qubits qs = {2, 9, 0, (int32_t)(k - 1), 12, 5, 7};
      if (r == 8) qs.push_back(10);
      RdmWidePlan p;
      rdm_wide_plan(k, r, qs.data(), &p, 8);
      CHECK(p.t.n_tiles / p.slices >= 2);
      const double d = model_pass(k, r, qs, 8, rng);
      CHECK(d < 1e-14);
      worst = std::max(worst, d);
    }
  std::printf("host model, r = 7..12: max |model - definition| = %.3e (bound 1e-14)\n", worst);
  // r <= 6: the plans, then the model up to k = 14 (8 tiles; with the cap at 3 a workgroup walks up to three of them)
  plans = 0;
  worst = 0;
  for (int r = 1; r <= 6; ++r) {
    std::vector<int> ks;
    for (int k = r; k <= r + 6; ++k) ks.push_back(k);
    for (int k : {14, 22, 23, 30}) ks.push_back(k);
    for (int k : ks)
      for (const Qubits& qs : placements(k, r, rng)) {
        for (int max_wg : {kRdmMaxWg, 3}) { check_narrow_plan(k, r, qs, max_wg); ++plans; }
        if (k > 14) continue;
        for (int max_wg : {kRdmMaxWg, 3}) {
          if (max_wg == 3 && k < 13) continue;       // (one tile: the same pass)
          const double d = model_narrow_pass(k, r, qs, max_wg, rng);
          CHECK(d < 1e-14);
          worst = std::max(worst, d);
        }
      }
  }
  std::printf("plans checked, r <= 6: %d\n", plans);
  std::printf("host model, r = 1..6: max |model - definition| = %.3e (bound 1e-14)\n", worst);
  if (g_failed) { std::printf("rdm_plan_check: %d FAILED\n", g_failed); return 1; }
  std::printf("rdm_plan_check: ok\n");
  return 0;
}
