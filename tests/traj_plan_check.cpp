// traj_plan_check.cpp -- stand-alone check of gs_traj_plan.h (the grouping of simulations into
// trajectory tables by size, probability and seed). Built with the host sanitizers and run
// directly by tests/test_traj_seeds_cpu.py; prints "ok".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gs_traj_plan.h"

#define CHECK(x)                                                    \
  do {                                                              \
    if (!(x)) {                                                     \
      std::fprintf(stderr, "line %d: %s\n", __LINE__, #x);          \
      std::exit(1);                                                 \
    }                                                               \
  } while (0)

static void check_perm(const gs::TrajPlan& pl, uint32_t n) {
  CHECK(pl.sim_of.size() == n && pl.slot_of.size() == n);
  std::vector<int> seen(n, 0);
  for (uint32_t s = 0; s < n; ++s) {
    CHECK(pl.sim_of[s] < n);
    seen[pl.sim_of[s]] += 1;
    CHECK(pl.slot_of[pl.sim_of[s]] == s);  // the inverse
  }
  for (uint32_t i = 0; i < n; ++i) CHECK(seen[i] == 1);
  uint32_t sum = 0;
  for (const gs::TrajPlanTab& t : pl.tabs) { CHECK(t.n_slots >= 1); sum += t.n_slots; }
  CHECK(sum == n);
}

int main() {
  {  // non-adjacent equal triples merge; tables in first-occurrence order; stable within a table
    const uint32_t sz[] = {12, 12, 16, 12, 12, 16};
    const double pr[] = {.05, .05, .05, .05, .25, .05};
    const uint64_t sd[] = {1, 2, 1, 1, 1, 1};
    const gs::TrajPlan pl = gs::traj_plan_build(6, sz, pr, sd, 99, .9, 99);
    check_perm(pl, 6);
    CHECK(pl.tabs.size() == 4 && pl.seeds_differ);
    CHECK(pl.tabs[0].asz == 12 && pl.tabs[0].p == .05 && pl.tabs[0].seed == 1 && pl.tabs[0].n_slots == 2);
    CHECK(pl.tabs[1].asz == 12 && pl.tabs[1].p == .05 && pl.tabs[1].seed == 2 && pl.tabs[1].n_slots == 1);
    CHECK(pl.tabs[2].asz == 16 && pl.tabs[2].p == .05 && pl.tabs[2].seed == 1 && pl.tabs[2].n_slots == 2);
    CHECK(pl.tabs[3].asz == 12 && pl.tabs[3].p == .25 && pl.tabs[3].seed == 1 && pl.tabs[3].n_slots == 1);
    const uint32_t want[] = {0, 3, 1, 2, 5, 4};
    for (uint32_t s = 0; s < 6; ++s) CHECK(pl.sim_of[s] == want[s]);
    const uint32_t inv[] = {0, 2, 3, 1, 5, 4};
    for (uint32_t i = 0; i < 6; ++i) CHECK(pl.slot_of[i] == inv[i]);
  }
  {  // one triple collapses to one table, the identity permutation
    const uint32_t sz[] = {8, 8, 8};
    const uint64_t sd[] = {5, 5, 5};
    const gs::TrajPlan pl = gs::traj_plan_build(3, sz, nullptr, sd, 12, .5, 7);
    check_perm(pl, 3);
    CHECK(pl.tabs.size() == 1 && !pl.seeds_differ);
    CHECK(pl.tabs[0].asz == 8 && pl.tabs[0].p == .5 && pl.tabs[0].seed == 5 && pl.tabs[0].n_slots == 3);
    for (uint32_t s = 0; s < 3; ++s) CHECK(pl.sim_of[s] == s);
  }
  {  // NULL columns fall back to the configuration's values
    const gs::TrajPlan pl = gs::traj_plan_build(4, nullptr, nullptr, nullptr, 12, .125, 42);
    check_perm(pl, 4);
    CHECK(pl.tabs.size() == 1 && pl.tabs[0].asz == 12 && pl.tabs[0].p == .125 && pl.tabs[0].seed == 42);
    const uint64_t sd[] = {3, 4, 3, 4};
    const gs::TrajPlan ps = gs::traj_plan_build(4, nullptr, nullptr, sd, 12, .125, 42);
    check_perm(ps, 4);
    CHECK(ps.tabs.size() == 2 && ps.seeds_differ);
    CHECK(ps.tabs[0].asz == 12 && ps.tabs[0].p == .125 && ps.tabs[0].seed == 3 && ps.tabs[0].n_slots == 2);
    CHECK(ps.tabs[1].asz == 12 && ps.tabs[1].p == .125 && ps.tabs[1].seed == 4 && ps.tabs[1].n_slots == 2);
    const uint32_t want[] = {0, 2, 1, 3};
    for (uint32_t s = 0; s < 4; ++s) CHECK(ps.sim_of[s] == want[s]);
    // sizes differ, seeds equal: several tables on one key
    const uint32_t sz[] = {6, 9, 6, 9};
    const gs::TrajPlan pz = gs::traj_plan_build(4, sz, nullptr, nullptr, 12, .125, 42);
    check_perm(pz, 4);
    CHECK(pz.tabs.size() == 2 && !pz.seeds_differ && pz.tabs[1].seed == 42 && pz.tabs[1].asz == 9);
  }
  {  // no sims
    const gs::TrajPlan pl = gs::traj_plan_build(0, nullptr, nullptr, nullptr, 12, .1, 1);
    CHECK(pl.tabs.empty() && pl.sim_of.empty() && pl.slot_of.empty() && !pl.seeds_differ);
  }
  std::puts("ok");
  return 0;
}
