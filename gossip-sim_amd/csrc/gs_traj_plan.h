// gs_traj_plan.h -- simulations to trajectory tables (plain C++, no device code: the whole-sim
// calls in gs_stats.cpp use it and tests/traj_plan_check.cpp checks it stand-alone).
//
// Every sim carries an active-set size, a rotation probability and a Philox seed; a NULL column
// takes the configuration's value for every sim. Sims of equal (size, probability, seed) share a
// table -- they need not be adjacent -- and the tables stand in the order of their first sim.
// The engine's slots are the sims in table order, stable within a table: sim_of[slot] is the
// slot's sim and slot_of[sim] its inverse.
#pragma once
#include <stdint.h>
#include <vector>

namespace gs {

struct TrajPlanTab {
  uint32_t asz;
  double p;
  uint64_t seed;
  uint32_t n_slots;
};

struct TrajPlan {
  std::vector<TrajPlanTab> tabs;
  std::vector<uint32_t> sim_of;   // [n_sims] slot -> sim
  std::vector<uint32_t> slot_of;  // [n_sims] sim -> slot
  bool seeds_differ = false;      // the tables do not all carry one seed
};

inline TrajPlan traj_plan_build(uint32_t n_sims, const uint32_t* sizes, const double* probs, const uint64_t* seeds,
                                uint32_t cfg_size, double cfg_prob, uint64_t cfg_seed) {
  TrajPlan pl;
  std::vector<uint32_t> tab_of(n_sims);
  for (uint32_t i = 0; i < n_sims; ++i) {
    const uint32_t a = sizes ? sizes[i] : cfg_size;
    const double p = probs ? probs[i] : cfg_prob;
    const uint64_t sd = seeds ? seeds[i] : cfg_seed;
    uint32_t t = 0;
    while (t < pl.tabs.size() && !(pl.tabs[t].asz == a && pl.tabs[t].p == p && pl.tabs[t].seed == sd)) ++t;
    if (t == pl.tabs.size()) pl.tabs.push_back(TrajPlanTab{a, p, sd, 0});
    pl.tabs[t].n_slots += 1;
    tab_of[i] = t;
  }
  pl.sim_of.reserve(n_sims);
  pl.slot_of.assign(n_sims, 0);
  for (uint32_t t = 0; t < pl.tabs.size(); ++t)
    for (uint32_t i = 0; i < n_sims; ++i)
      if (tab_of[i] == t) {
        pl.slot_of[i] = (uint32_t)pl.sim_of.size();
        pl.sim_of.push_back(i);
      }
  for (const TrajPlanTab& t : pl.tabs) pl.seeds_differ = pl.seeds_differ || t.seed != pl.tabs[0].seed;
  return pl;
}

}  // namespace gs
