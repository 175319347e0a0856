// split_plan_check.cpp -- stand-alone check of gs_split_plan.h (the generations of the round
// split: which row / rotation-list generation each round reads and writes, and which launches a
// launch waits for). Built with the host sanitizers and run directly by
// tests/test_round_split_cpu.py; prints "ok".
//
// Three things are checked over 12 rounds, with joins and resets at arbitrary points:
//  1. the arithmetic: without a reset round k reads generation k % 3, its rotation writes
//     (k + 1) % 3 and list k % 3, and the catch-up names lists (k - 1) % 3 and (k - 2) % 3;
//  2. no hazard: under the event dependencies (group 0's round k after group 1's k - 2, group 1's
//     round k after group 0's k - 1, each stream in order) nothing a launch writes is read or
//     written by a launch that may still run;
//  3. the contents: a model of the rows (a value per node and generation) driven by the plan --
//     copy the two named lists' nodes from `read` to `write`, then rotate there -- gives every
//     round exactly the rows a single buffer rotated in place gives.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gs_split_plan.h"

#define CHECK(x)                                                    \
  do {                                                              \
    if (!(x)) {                                                     \
      std::fprintf(stderr, "line %d: %s\n", __LINE__, #x);          \
      std::exit(1);                                                 \
    }                                                               \
  } while (0)

namespace {

constexpr int ROUNDS = 12, NODES = 41;

// which nodes rotation r touches (about a third, so consecutive lists overlap), and what it does
bool rotates(uint32_t r, int u) { return ((uint32_t)u * 2654435761u + r * 40503u) % 3u == 0; }
uint64_t rotated(uint64_t old, uint32_t r, int u) { return old * 6364136223846793005ull + r * 1442695040888963407ull + (uint64_t)u; }

struct Launch {  // what one group's launch of a round touches
  int rows_read = -1, rows_write = -1;
  int lists_read[2] = {-1, -1};  // the pending clear's (= catch1) and catch2's
  int list_write = -1;
};

bool conflicts(const Launch& w, const Launch& o) {  // w's writes against o's reads and writes
  if (w.rows_write >= 0 && (w.rows_write == o.rows_read || w.rows_write == o.rows_write)) return true;
  if (w.list_write >= 0)
    if (w.list_write == o.lists_read[0] || w.list_write == o.lists_read[1] || w.list_write == o.list_write) return true;
  return false;
}

// events[i]: 0 nothing, 1 a join before round i, 2 a join and an in-place row change (reset) before round i
void run(const int (&events)[ROUNDS]) {
  gs::SplitPlan pl;
  std::vector<uint64_t> ref(NODES), gen[3];
  for (int u = 0; u < NODES; ++u) ref[u] = 1000 + u;
  for (auto& g : gen) g.assign(NODES, 0);  // (stale until the first reset)
  std::vector<int> lists[3];
  std::vector<Launch> g0(ROUNDS), g1(ROUNDS);
  int done_before = 0;   // rounds below this index have ended (a join)
  int since_reset = 0;   // index of the first round after the last reset
  bool live = false;
  for (int i = 0; i < ROUNDS; ++i) {
    if (events[i]) done_before = i;
    if (events[i] == 2 || !live) {  // the rows changed in place: whole copies, all generations equal
      if (events[i] == 2)
        for (int u = 0; u < NODES; u += 5) ref[u] += 77 + i;  // (an uploaded entry, say)
      const int cur = live ? pl.cur : 0;
      gen[cur] = ref;
      CHECK(done_before == i || i == 0);  // a reset joins first
      for (auto& g : gen) g = ref;
      pl.reset(cur);
      since_reset = i;
      live = true;
    }
    const int64_t k = pl.k;
    const gs::SplitStep s = pl.next();
    CHECK(k == i - since_reset);
    // 1. the arithmetic
    CHECK(s.read >= 0 && s.read < 3 && s.write >= 0 && s.write < 3 && s.list >= 0 && s.list < 3);
    CHECK(s.write != s.read);
    if (since_reset == 0 && events[i] != 2) {
      CHECK(s.read == k % 3 && s.write == (k + 1) % 3 && s.list == k % 3);
      CHECK(s.catch1 == (k >= 1 ? (int)((k - 1) % 3) : -1));
      CHECK(s.catch2 == (k >= 2 ? (int)((k - 2) % 3) : -1));
    }
    CHECK(s.catch1 == (k >= 1 ? g0[i - 1].list_write : -1));  // the last rotation's list
    CHECK(s.catch2 == (k >= 2 ? g0[i - 2].list_write : -1));
    CHECK(s.list != s.catch1 && s.list != s.catch2);
    CHECK(s.g0_waits_g1 == (k >= 2 ? k - 2 : -1) && s.g1_waits_g0 == (k >= 1 ? k - 1 : -1));
    if (k >= 1) CHECK(s.read == g0[i - 1].rows_write);  // the rows the last rotation left
    g0[i].rows_read = s.read; g0[i].rows_write = s.write;
    g0[i].lists_read[0] = s.catch1; g0[i].lists_read[1] = s.catch2; g0[i].list_write = s.list;
    g1[i].rows_read = s.read; g1[i].lists_read[0] = s.catch1;
    // 2. what may still run when group 0's round i runs: every round of group 1 since the last
    // join, but those up to the one it waits for (group 1's stream runs them in order); group 0's
    // earlier rounds are on its own stream. Without a join these are group 1's rounds i - 1 and i.
    int may_run = 0;
    for (int j = done_before; j <= i; ++j) {
      if (s.g0_waits_g1 >= 0 && j - since_reset <= s.g0_waits_g1) continue;
      CHECK(!conflicts(g0[i], g1[j]));
      ++may_run;
    }
    CHECK(may_run >= 1 && may_run <= 2);
    // ... and when group 1's round i runs: group 0's rounds i and i + 1 (checked from their side,
    // above and at the next trip); group 0's round i - 1, which wrote what it reads, has ended:
    if (k >= 1) CHECK(s.g1_waits_g0 == k - 1 && g0[i - 1].rows_write == g1[i].rows_read);
    // 3. the contents: the slots of round i read the rows a single buffer would hold
    CHECK(gen[s.read] == ref);
    for (int q = 0; q < 2; ++q) {
      const int lg = q ? s.catch2 : s.catch1;
      if (lg < 0) continue;
      for (int u : lists[lg]) gen[s.write][u] = gen[s.read][u];
    }
    CHECK(gen[s.write] == ref);  // (equal before the rotation: nothing else differed)
    lists[s.list].clear();
    for (int u = 0; u < NODES; ++u)
      if (rotates((uint32_t)i, u)) {
        lists[s.list].push_back(u);
        gen[s.write][u] = rotated(gen[s.write][u], (uint32_t)i, u);
        ref[u] = rotated(ref[u], (uint32_t)i, u);
      }
    CHECK(gen[s.write] == ref);
    CHECK(pl.cur == s.write && pl.prev == s.read && pl.p1 == s.list && pl.p2 == s.catch1);
  }
}

}  // namespace

int main() {
  const int none[ROUNDS] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  run(none);
  const int joins[ROUNDS] = {0, 0, 0, 1, 0, 0, 1, 1, 0, 0, 0, 1};  // readbacks mid-run
  run(joins);
  const int resets[ROUNDS] = {0, 2, 0, 0, 0, 1, 0, 2, 2, 0, 0, 0};  // rows changed in place
  run(resets);
  const int mixed[ROUNDS] = {2, 0, 1, 0, 2, 0, 0, 1, 0, 0, 2, 1};
  run(mixed);
  // every pattern of one reset and one join
  for (int a = 0; a < ROUNDS; ++a)
    for (int b = 0; b < ROUNDS; ++b) {
      int ev[ROUNDS] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
      ev[b] = 1;
      ev[a] = 2;
      run(ev);
    }
  std::printf("ok\n");
  return 0;
}
