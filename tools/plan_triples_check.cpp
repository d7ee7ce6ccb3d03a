// Stand-alone host check of the line-qubit triple search (quantum_simulations_amd/csrc/tile_search.h plan_search_triples,
// qsim_plan_search_triples): on a seeded 12-qubit and a seeded 14-qubit random 1q + CX list,
//   * the bounded call over all C(n, 3) triples returns exactly the fewest passes, the triples and the masks that unbounded
//     one-triple searches (qsim_plan_search on the list relabelled here, by the documented rule) give, and the count of its
//     histogram at the fewest passes;
//   * the result -- with the plain bound, with the bound that counts needed tile bits, and unbounded -- is identical with
//     1, 3 and 16 threads.
// No device is touched: every call is a host-only planning call.  The planner is part of the library's single translation
// unit, which includes the HIP runtime header, so this file includes that unit and is compiled by hipcc with the sanitizer
// on the host side only; the program has its own main and needs no GPU:
//   hipcc -x hip --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=all tools/plan_triples_check.cpp -o plan_triples_check && ./plan_triples_check
//   (once with -Xarch_host -fsanitize=thread in place of address,undefined)
// Exit status 0 and a last line "plan_triples_check: ok" mean that every case passed.
#include "../quantum_simulations_amd/csrc/qsim_hip.hip"

#include <random>

static int g_failed = 0;
#define CHECK(cond)                                                              \
  do {                                                                           \
    if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_failed; } \
  } while (0)

struct OpList {
  std::vector<int32_t> nq, qubits;
  std::vector<double> mats;                      // 32 doubles per op (row-major complex 4x4; a 1q gate uses the first 8)
  int size() const { return (int)nq.size(); }
};

// layers of random SU(2) gates on every qubit, then CNOTs on a random pairing
static OpList random_list(int n, int layers, unsigned seed) {
  std::mt19937_64 rng(seed);
  std::uniform_real_distribution<double> angle(0.0, 6.283185307179586);
  OpList l;
  auto push = [&](int nq, int a, int b, const std::vector<double>& m) {
    l.nq.push_back(nq);
    l.qubits.push_back(a);
    l.qubits.push_back(b);
    l.mats.insert(l.mats.end(), m.begin(), m.end());
    l.mats.resize((size_t)32 * l.nq.size(), 0.0);
  };
  for (int layer = 0; layer < layers; ++layer) {
    for (int q = 0; q < n; ++q) {
      const double t = angle(rng) / 2, p = angle(rng), s = angle(rng);
      push(1, q, 0, {std::cos(t), 0, -std::cos(s) * std::sin(t), -std::sin(s) * std::sin(t),
                     std::cos(p) * std::sin(t), std::sin(p) * std::sin(t), std::cos(p + s) * std::cos(t), std::sin(p + s) * std::cos(t)});
    }
    std::vector<int> order((size_t)n);
    for (int q = 0; q < n; ++q) order[(size_t)q] = q;
    std::shuffle(order.begin(), order.end(), rng);
    for (int i = 0; i + 1 < n; i += 2) {
      std::vector<double> cx(32, 0.0);           // |c t>: control = first qubit (the high bit of the 4x4's index)
      cx[2 * (0 * 4 + 0)] = cx[2 * (1 * 4 + 1)] = cx[2 * (2 * 4 + 3)] = cx[2 * (3 * 4 + 2)] = 1.0;
      push(2, order[(size_t)i], order[(size_t)i + 1], cx);
    }
  }
  return l;
}

struct Found {
  int best = -1, n_found = 0;
  std::vector<int32_t> index, triples, histogram;
  std::vector<uint64_t> masks;
  bool operator==(const Found& o) const {
    return best == o.best && n_found == o.n_found && index == o.index && triples == o.triples && masks == o.masks;
  }
};

static Found search_all(int n, const OpList& l, int threads, int flags) {
  const size_t m = (size_t)n * (n - 1) * (n - 2) / 6;
  Found f;
  f.index.assign(m, -1);
  f.triples.assign(3 * m, -1);
  f.histogram.assign(QSIM_PLAN_HISTOGRAM_BINS, -1);
  f.masks.assign(m * (size_t)l.size(), 0);
  int32_t best = -1, count = -1;
  const int rc = qsim_plan_search_triples(n, l.size(), l.nq.data(), l.qubits.data(), l.mats.data(), 0, nullptr, 0, threads, flags, &best,
                                          &count, f.index.data(), f.triples.data(), f.masks.data(), f.masks.size(), f.histogram.data());
  CHECK(rc == QSIM_OK);
  if (rc != QSIM_OK) return f;
  f.best = best;
  f.n_found = count;
  f.index.resize((size_t)count);
  f.triples.resize(3 * (size_t)count);
  f.masks.resize((size_t)count * (size_t)best);
  return f;
}

static void check_size(int n, int layers, unsigned seed) {
  const OpList l = random_list(n, layers, seed);
  // the reference: every triple on its own, relabelled here, through the one-triple call
  Found want;
  std::vector<int> passes;
  std::vector<std::vector<uint64_t>> masks;
  std::vector<int32_t> all;
  for (int a = 0; a < n; ++a)
    for (int b = a + 1; b < n; ++b)
      for (int c = b + 1; c < n; ++c) {
        const int32_t t[3] = {a, b, c};
        std::vector<int32_t> lay((size_t)n), q(l.qubits.size());
        for (int i = 0; i < n; ++i) lay[(size_t)i] = i;
        for (int bit = 0; bit < 3; ++bit) {        // the qubit on line bit `bit` trades places with t[bit]
          const int j = (int)(std::find(lay.begin(), lay.end(), bit) - lay.begin());
          lay[(size_t)j] = lay[(size_t)t[bit]];
          lay[(size_t)t[bit]] = bit;
        }
        for (size_t i = 0; i < q.size(); ++i) q[i] = (i % 2 == 0 || l.nq[i / 2] == 2) ? lay[(size_t)l.qubits[i]] : 0;
        std::vector<uint64_t> out((size_t)l.size());
        int32_t count = -1;
        CHECK(qsim_plan_search(n, l.size(), l.nq.data(), q.data(), l.mats.data(), 0, out.data(), (int)out.size(), &count) == QSIM_OK);
        out.resize((size_t)std::max(count, 0));
        passes.push_back(count);
        masks.push_back(out);
        all.insert(all.end(), t, t + 3);
      }
  want.best = *std::min_element(passes.begin(), passes.end());
  for (size_t t = 0; t < passes.size(); ++t)
    if (passes[t] == want.best) {
      ++want.n_found;
      want.index.push_back((int32_t)t);
      want.triples.insert(want.triples.end(), all.begin() + 3 * (long)t, all.begin() + 3 * (long)t + 3);
      want.masks.insert(want.masks.end(), masks[t].begin(), masks[t].end());
    }
  std::vector<int> spread(QSIM_PLAN_HISTOGRAM_BINS, 0);
  for (int p : passes) ++spread[(size_t)std::min(p, QSIM_PLAN_HISTOGRAM_BINS - 2)];
  std::printf("n = %d: %d ops, %zu triples, fewest passes %d on %d of them\n", n, l.size(), passes.size(), want.best, want.n_found);
  // (at 12 qubits a tile leaves one qubit out and every triple ties; at 14 the bound has something to cut)
  if (n >= 14) CHECK(want.best >= 2 && want.n_found < (int)passes.size());
  const int thread_counts[3] = {1, 3, 16};
  const int flag_sets[3] = {0, QSIM_TRIPLES_NEED_BITS, QSIM_TRIPLES_UNBOUNDED};
  for (int flags : flag_sets)
    for (int threads : thread_counts) {
      const Found got = search_all(n, l, threads, flags);
      CHECK(got == want);
      CHECK(got.histogram[(size_t)want.best] == want.n_found);
      for (int p = 0; p < want.best; ++p) CHECK(got.histogram[(size_t)p] == 0);
      long total = 0;
      for (int32_t c : got.histogram) total += c;
      CHECK(total == (long)passes.size());
      if (flags & QSIM_TRIPLES_UNBOUNDED)
        for (int p = 0; p < QSIM_PLAN_HISTOGRAM_BINS - 1; ++p) CHECK(got.histogram[(size_t)p] == spread[(size_t)p]);
      else
        CHECK(got.histogram[QSIM_PLAN_HISTOGRAM_BINS - 1] == (int)passes.size() - want.n_found);
    }
}

int main() {
  check_size(12, 10, 12u);
  check_size(14, 10, 14u);
  // what the call refuses: a repeated qubit, a qubit outside the register, too small a buffer
  const OpList l = random_list(12, 4, 1u);
  int32_t best = 0, count = 0, index[2], found[6];
  uint64_t masks[64];
  const int32_t twice[3] = {4, 7, 4}, outside[3] = {0, 1, 12}, fine[6] = {0, 1, 2, 5, 3, 9};
  CHECK(qsim_plan_search_triples(12, l.size(), l.nq.data(), l.qubits.data(), l.mats.data(), 1, twice, 0, 1, 0, &best, &count, index, found, masks, 64, nullptr) == QSIM_ERR_INVALID);
  CHECK(qsim_plan_search_triples(12, l.size(), l.nq.data(), l.qubits.data(), l.mats.data(), 1, outside, 0, 1, 0, &best, &count, index, found, masks, 64, nullptr) == QSIM_ERR_INVALID);
  CHECK(qsim_plan_search_triples(12, l.size(), l.nq.data(), l.qubits.data(), l.mats.data(), 2, fine, 0, 2, 0, &best, &count, index, found, masks, 0, nullptr) == QSIM_ERR_INVALID);
  CHECK(qsim_plan_search_triples(12, l.size(), l.nq.data(), l.qubits.data(), l.mats.data(), 2, fine, 0, 2, 0, &best, &count, index, found, masks, 64, nullptr) == QSIM_OK);
  CHECK(best >= 1 && count >= 1 && count <= 2);
  if (g_failed) { std::printf("plan_triples_check: %d check(s) FAILED\n", g_failed); return 1; }
  std::printf("plan_triples_check: ok\n");
  return 0;
}
