// Stand-alone host check of the cyclic-plan search (quantum_simulations_amd/csrc/tile_search.h plan_search_cycle,
// qsim_plan_search_cycle) and of the host side of the cycle object (qsim_cycle_create): on a seeded 12-qubit and a seeded
// 14-qubit random 1q + CX list, over all C(n, 3) line-qubit triples,
//   * the cut: head and tail of every returned cycle partition the list, neither is empty, and the steady passes are the
//     same for all of them and fewer than the plain ones, which are what qsim_plan_search gives under the triple;
//   * the replay: head, tail . head and tail, built here from the tail bytes and relabelled here by the documented rule, plan
//     through the hint path (qsim_plan_ops_tiled) into exactly the passes counted, and qsim_cycle_create prepares as many;
//   * the result is identical with 1, 3 and 16 threads, and with the plain passes handed in instead of searched.
// No device is touched.  Built and run like tools/plan_triples_check.cpp (the library's translation unit included, hipcc
// with the sanitizer on the host side only, a main of its own):
//   hipcc -x hip --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=all tools/plan_cycle_check.cpp -o plan_cycle_check && ./plan_cycle_check
//   (once with -Xarch_host -fsanitize=thread in place of address,undefined)
// Exit status 0 and a last line "plan_cycle_check: ok" mean that every case passed.
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
  void push(const OpList& from, int i, const std::vector<int32_t>& lay) {
    nq.push_back(from.nq[(size_t)i]);
    qubits.push_back(lay[(size_t)from.qubits[2 * (size_t)i]]);
    qubits.push_back(from.nq[(size_t)i] == 2 ? lay[(size_t)from.qubits[2 * (size_t)i + 1]] : 0);
    mats.insert(mats.end(), from.mats.begin() + 32 * (long)i, from.mats.begin() + 32 * (long)i + 32);
  }
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

struct Cycles {
  int n_found = -1;
  std::vector<int32_t> index, triples, passes;
  std::vector<uint8_t> tail;
  std::vector<uint64_t> masks;
  bool operator==(const Cycles& o) const {
    return n_found == o.n_found && index == o.index && triples == o.triples && passes == o.passes && tail == o.tail && masks == o.masks;
  }
};

static Cycles search(int n, const OpList& l, const std::vector<int32_t>& triples, const int32_t* plain, int threads) {
  const size_t m = triples.size() / 3;
  Cycles c;
  c.index.assign(m, -1);
  c.triples.assign(3 * m, -1);
  c.passes.assign(4 * m, -1);
  c.tail.assign(m * (size_t)l.size(), 255);
  c.masks.assign(3 * m * (size_t)l.size(), 0);
  int32_t count = -1;
  const int rc = qsim_plan_search_cycle(n, l.size(), l.nq.data(), l.qubits.data(), l.mats.data(), (int)m, triples.data(), plain, 0, threads,
                                        &count, c.index.data(), c.triples.data(), c.passes.data(), c.tail.data(), c.masks.data(), c.masks.size());
  CHECK(rc == QSIM_OK);
  if (rc != QSIM_OK) return c;
  c.n_found = count;
  size_t used = 0;
  for (int f = 0; f < count; ++f) used += (size_t)(c.passes[4 * (size_t)f + 1] + c.passes[4 * (size_t)f + 2] + c.passes[4 * (size_t)f + 3]);
  c.index.resize((size_t)count);
  c.triples.resize(3 * (size_t)count);
  c.passes.resize(4 * (size_t)count);
  c.tail.resize((size_t)count * (size_t)l.size());
  c.masks.resize(used);
  return c;
}

static void check_size(int n, int layers, unsigned seed) {
  const OpList l = random_list(n, layers, seed);
  std::vector<int32_t> all;
  for (int a = 0; a < n; ++a)
    for (int b = a + 1; b < n; ++b)
      for (int c = b + 1; c < n; ++c) { all.push_back(a); all.push_back(b); all.push_back(c); }
  const Cycles want = search(n, l, all, nullptr, 1);
  std::printf("n = %d: %d ops, %zu triples, %d cycles", n, l.size(), all.size() / 3, want.n_found);
  if (want.n_found > 0) std::printf(" (plain %d: head %d, steady %d, tail %d)", want.passes[0], want.passes[1], want.passes[2], want.passes[3]);
  std::printf("\n");
  size_t at = 0;
  for (int f = 0; f < want.n_found; ++f) {
    const int32_t* t = &want.triples[3 * (size_t)f];
    const int32_t* p = &want.passes[4 * (size_t)f];
    const uint8_t* late = &want.tail[(size_t)f * (size_t)l.size()];
    CHECK(want.index[(size_t)f] >= 0 && std::equal(t, t + 3, &all[3 * (size_t)want.index[(size_t)f]]));
    CHECK(p[2] < p[0] && p[2] == want.passes[2]);
    std::vector<int32_t> lay((size_t)n);
    for (int i = 0; i < n; ++i) lay[(size_t)i] = i;
    for (int bit = 0; bit < 3; ++bit) {          // the qubit on line bit `bit` trades places with t[bit]
      const int j = (int)(std::find(lay.begin(), lay.end(), bit) - lay.begin());
      lay[(size_t)j] = lay[(size_t)t[bit]];
      lay[(size_t)t[bit]] = bit;
    }
    OpList whole, head, tail;
    for (int i = 0; i < l.size(); ++i) {
      CHECK(late[i] <= 1);
      whole.push(l, i, lay);
      (late[i] ? tail : head).push(l, i, lay);
    }
    CHECK(head.size() > 0 && tail.size() > 0 && head.size() + tail.size() == l.size());
    OpList steady = tail;
    for (int i = 0; i < l.size(); ++i) if (!late[i]) steady.push(l, i, lay);
    std::vector<uint64_t> out((size_t)l.size());
    int32_t plain = -1;
    CHECK(qsim_plan_search(n, whole.size(), whole.nq.data(), whole.qubits.data(), whole.mats.data(), 0, out.data(), (int)out.size(), &plain) == QSIM_OK);
    CHECK(plain == p[0]);
    const OpList* parts[3] = {&head, &steady, &tail};
    qsim_cycle_list lists[3];
    for (int w = 0; w < 3; ++w) {
      const OpList& part = *parts[w];
      int32_t replayed = -1;
      CHECK(qsim_plan_ops_tiled(n, part.size(), part.nq.data(), part.qubits.data(), part.mats.data(), p[1 + w], &want.masks[at], nullptr, 0, &replayed) == QSIM_OK);
      CHECK(replayed == p[1 + w]);
      lists[w] = qsim_cycle_list{part.size(), part.nq.data(), part.qubits.data(), part.mats.data(), p[1 + w], &want.masks[at], nullptr};
      at += (size_t)p[1 + w];
    }
    qsim_cycle* cycle = nullptr;
    int32_t prepared[3] = {-1, -1, -1};
    CHECK(qsim_cycle_create(n, &lists[0], &lists[1], &lists[2], prepared, &cycle) == QSIM_OK);
    CHECK(cycle && prepared[0] == p[1] && prepared[1] == p[2] && prepared[2] == p[3]);
    CHECK(qsim_cycle_destroy(cycle) == QSIM_OK);
  }
  CHECK(at == want.masks.size());
  for (int threads : {3, 16}) CHECK(search(n, l, all, nullptr, threads) == want);
  // the plain passes handed in (those of the found triples: every one of them reaches the same count)
  if (want.n_found > 0) {
    const std::vector<int32_t> plain((size_t)want.n_found, want.passes[0]);
    Cycles again = search(n, l, want.triples, plain.data(), 4);
    CHECK(again.n_found == want.n_found && again.triples == want.triples && again.passes == want.passes && again.tail == want.tail && again.masks == want.masks);
  }
}

int main() {
  check_size(12, 10, 12u);
  check_size(14, 10, 14u);
  // what the calls refuse: no triple, a repeated qubit, too small a buffer, a cycle with an empty list
  const OpList l = random_list(12, 6, 1u);
  int32_t count = 0, index[2], found[6], passes[8];
  std::vector<uint8_t> tail(2 * (size_t)l.size());
  uint64_t masks[256];
  const int32_t twice[3] = {4, 7, 4}, fine[6] = {0, 1, 2, 5, 3, 9};
  CHECK(qsim_plan_search_cycle(12, l.size(), l.nq.data(), l.qubits.data(), l.mats.data(), 0, fine, nullptr, 0, 1, &count, index, found, passes, tail.data(), masks, 256) == QSIM_ERR_INVALID);
  CHECK(qsim_plan_search_cycle(12, l.size(), l.nq.data(), l.qubits.data(), l.mats.data(), 1, twice, nullptr, 0, 1, &count, index, found, passes, tail.data(), masks, 256) == QSIM_ERR_INVALID);
  CHECK(qsim_plan_search_cycle(12, l.size(), l.nq.data(), l.qubits.data(), l.mats.data(), 2, fine, nullptr, 0, 2, &count, index, found, passes, tail.data(), masks, 256) == QSIM_OK);
  if (count > 0)
    CHECK(qsim_plan_search_cycle(12, l.size(), l.nq.data(), l.qubits.data(), l.mats.data(), 2, fine, nullptr, 0, 2, &count, index, found, passes, tail.data(), masks, 0) == QSIM_ERR_INVALID);
  const qsim_cycle_list whole = {l.size(), l.nq.data(), l.qubits.data(), l.mats.data(), 0, nullptr, nullptr};
  const qsim_cycle_list empty = {0, nullptr, nullptr, nullptr, 0, nullptr, nullptr};
  qsim_cycle* cycle = nullptr;
  CHECK(qsim_cycle_create(12, &whole, &whole, &empty, nullptr, &cycle) == QSIM_ERR_INVALID && !cycle);
  CHECK(qsim_cycle_create(12, &whole, &whole, &whole, nullptr, &cycle) == QSIM_OK && cycle);
  CHECK(qsim_cycle_destroy(cycle) == QSIM_OK);
  if (g_failed) { std::printf("plan_cycle_check: %d check(s) FAILED\n", g_failed); return 1; }
  std::printf("plan_cycle_check: ok\n");
  return 0;
}
