// cluster_plan_check.cpp -- stand-alone check of gs_cluster_plan.h (the slot chunks of the grouped
// cluster load view: blockIdx.y of its reduction indexes this table, and a block sums its chunk's
// slots into ONE group's scratch). Built plainly and with the host sanitizers and run directly by
// tests/test_cluster_groups_cpu.py; prints "ok".
//
// For every case (NP, group sizes):
//  1. every chunk lies in one group: [s_lo, s_hi) within the slots [a_g, a_g + n_g) of its group;
//  2. the chunks of a group tile it exactly once, in slot order (so every slot of the engine is
//     counted once, and for its own group);
//  3. no chunk is empty, and none is longer than the plan's chunk size, a multiple of 16;
//  4. the chunk count is within the stated bound: G <= chunks <= want + G, where
//     want = max(1, ceil(2,048 / node blocks)) is the count the ungrouped view aims for;
//  5. with one group the chunks are exactly the ungrouped view's (CH slots each from slot 0).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <vector>

#include "gs_cluster_plan.h"

#define CHECK(x)                                                    \
  do {                                                              \
    if (!(x)) {                                                     \
      std::fprintf(stderr, "line %d: %s (case %d)\n", __LINE__, #x, g_case); \
      std::exit(1);                                                 \
    }                                                               \
  } while (0)

namespace {

int g_case = 0;

void check(uint32_t NP, const std::vector<uint32_t>& sizes) {
  ++g_case;
  const uint32_t G = (uint32_t)sizes.size();
  const uint64_t S = std::accumulate(sizes.begin(), sizes.end(), (uint64_t)0);
  const std::vector<gs::ClusterChunk> plan = gs::cluster_plan_build(NP, sizes.data(), G);
  const uint32_t chunk = gs::cluster_plan_chunk(NP, (uint32_t)S), want = gs::cluster_plan_want(NP);
  CHECK(chunk >= 16 && chunk % 16 == 0);
  CHECK((uint64_t)chunk * want >= S);  // want full chunks cover the slots
  std::vector<uint32_t> start(G + 1, 0);
  for (uint32_t g = 0; g < G; ++g) start[g + 1] = start[g] + sizes[g];
  std::vector<uint32_t> covered(S, 0);   // times each slot is taken
  std::vector<uint32_t> next(start.begin(), start.end() - 1);  // where each group's next chunk must begin
  uint32_t last_group = 0;
  for (const gs::ClusterChunk& c : plan) {
    CHECK(c.group < G);
    CHECK(c.group >= last_group);  // groups in order
    last_group = c.group;
    CHECK(c.s_lo < c.s_hi);                                            // 3. not empty
    CHECK(c.s_hi - c.s_lo <= chunk);
    CHECK(c.s_lo >= start[c.group] && c.s_hi <= start[c.group + 1]);   // 1. in one group
    CHECK(c.s_lo == next[c.group]);                                    // 2. contiguous, in order
    next[c.group] = c.s_hi;
    for (uint32_t j = c.s_lo; j < c.s_hi; ++j) ++covered[j];
  }
  for (uint32_t g = 0; g < G; ++g) CHECK(next[g] == start[g + 1]);     // 2. to the group's end
  for (uint64_t j = 0; j < S; ++j) CHECK(covered[j] == 1);             // 2. exactly once
  CHECK(plan.size() >= G && plan.size() <= (size_t)want + G);          // 4.
  if (G == 1) {                                                        // 5.
    CHECK(plan.size() == (S + chunk - 1) / chunk);
    for (size_t k = 0; k < plan.size(); ++k) CHECK(plan[k].s_lo == k * chunk);
  }
}

}  // namespace

int main() {
  const uint32_t NPS[] = {1, 3, 67, 131, 256, 257, 1025, 3000, 1000000, 10000000};
  for (uint32_t NP : NPS) {
    check(NP, {7});                                    // G = 1
    check(NP, {1});                                    // ... of one slot
    check(NP, std::vector<uint32_t>(7, 1));            // G = S
    check(NP, {3, 1, 3});
    check(NP, {1, 64, 5});
    check(NP, {17, 17, 17, 19});
    check(NP, {3000});                                 // one group of 3,000
    check(NP, std::vector<uint32_t>(16, 1));           // 16 tables of 1
    check(NP, {2, 3});
    check(NP, {1500, 1, 1499});
    check(NP, std::vector<uint32_t>(3000, 1));
    check(NP, {33, 16, 15, 17, 4000, 31});
  }
  std::puts("ok");
  return 0;
}
