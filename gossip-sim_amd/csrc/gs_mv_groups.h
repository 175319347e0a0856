// gs_mv_groups.h -- the slot groups of the multi-source BFS and their tables, built on the host.
// Plain C++ (no HIP types), so the builder can be compiled and checked on its own.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#if defined(__HIPCC__)
#define GS_MV_HD __host__ __device__
#else
#define GS_MV_HD
#endif

namespace gs {

constexpr uint32_t MV_NB = 25;  // NUM_PUSH_ACTIVE_SET_ENTRIES (push_active_set.rs:11; = NB of gs_device.h)

// A group's table. Words [0, GT_WORDS) are what the level kernels copy to LDS: per entry k the
// group's slots whose origin bucket is >= k (GT_OWN), the distinct origin buckets and their slot
// masks (GT_NOBS, GT_OBV, GT_OBM), the seed range and the slot range.
constexpr uint32_t GT_WORDS = 96;
constexpr uint32_t GT_OWN = 0, GT_NOBS = 25, GT_OBV = 26, GT_OBM = 58, GT_NSEED = 90, GT_SEED = 91, GT_S0 = 92,
                   GT_SG = 93;
// ... followed by the group's origin -> slot-mask hash (128 (id, mask) pairs, two probes;
// word GT_OTOK of the table = 1 when every origin is in it)
constexpr uint32_t GT_OT = GT_WORDS, GT_OTOK = 94;
// ... and by the group's trajectory tables (engines of several tables): the number of
// tables with a slot in the group (GT_NT), then per such table its index (GT_TI) and the mask of
// the group's slots it serves (GT_TM; the masks partition the group's slots). The level kernels
// of several-table engines read these words from global memory, so the LDS part keeps its size
// and the single-table kernels their LDS. A group's table is GT_STRIDE words.
constexpr uint32_t GT_NT = GT_OT + 256, GT_TI = GT_NT + 1, GT_TM = GT_TI + 28, GT_STRIDE = GT_OT + 256 + 64;
constexpr uint32_t MV_GW_MAX = 28;  // slots per group at most (mv_geometry)

struct MvGroup { uint32_t s0, sg, seed0, nseed; };
struct MvSeed { uint32_t x, y; };  // a frontier entry: node | entry << 24, slot mask (the layout of uint2)

GS_MV_HD inline uint32_t mv_ohash(uint32_t x) { return (x * 0x9E3779B1u) >> 25; }

// Slot groups (contiguous ranges of <= GW slots, independent of the trajectory tables) and their
// tables. origins / obkt: per slot; bucket: per node; stab: each slot's trajectory table (null:
// one table). Seeds: one level-0 entry per distinct (origin, table) of a group -- a frontier
// entry's slots share one table -- at the origin's own entry.
inline void mv_groups_build(uint32_t S, uint32_t GW, const uint32_t* origins, const uint8_t* obkt,
                            const uint8_t* bucket, const uint32_t* stab, std::vector<uint32_t>& gtab,
                            std::vector<MvSeed>& seeds, std::vector<MvGroup>& groups) {
  const uint32_t ng = (S + GW - 1) / GW;
  gtab.assign((size_t)ng * GT_STRIDE, 0);
  seeds.clear();
  groups.clear();
  for (uint32_t g = 0; g < ng; ++g) {
    const uint32_t s0 = g * GW, sg = std::min(GW, S - s0);
    uint32_t* t = gtab.data() + (size_t)g * GT_STRIDE;
    {  // origin -> slot mask, open addressing with two probes (mv_origin_slots)
      uint32_t* ot = t + GT_OT;
      for (uint32_t i = 0; i < 128; ++i) ot[2 * i] = 0xFFFFFFFFu;
      bool ok = true;
      for (uint32_t j = 0; j < sg; ++j) {
        const uint32_t o = origins[s0 + j], h0 = mv_ohash(o), h1 = (h0 + 1) & 127u;
        const uint32_t h = (ot[2 * h0] == o || ot[2 * h0] == 0xFFFFFFFFu) ? h0
                           : (ot[2 * h1] == o || ot[2 * h1] == 0xFFFFFFFFu) ? h1 : 128u;
        if (h == 128u) { ok = false; continue; }
        ot[2 * h] = o;
        ot[2 * h + 1] |= 1u << j;
      }
      t[GT_OTOK] = ok ? 1u : 0u;
    }
    for (uint32_t k = 0; k < MV_NB; ++k)
      for (uint32_t j = 0; j < sg; ++j)
        if (obkt[s0 + j] >= k) t[GT_OWN + k] |= 1u << j;
    uint32_t nobs = 0;
    for (uint32_t j = 0; j < sg; ++j) {
      uint32_t i = 0;
      while (i < nobs && t[GT_OBV + i] != obkt[s0 + j]) ++i;
      if (i == nobs) { t[GT_OBV + i] = obkt[s0 + j]; ++nobs; }
      t[GT_OBM + i] |= 1u << j;
    }
    t[GT_NOBS] = nobs;
    uint32_t nt = 0;  // the tables with a slot in this group, in slot order
    for (uint32_t j = 0; j < sg; ++j) {
      const uint32_t tb = stab ? stab[s0 + j] : 0u;
      uint32_t i = 0;
      while (i < nt && t[GT_TI + i] != tb) ++i;
      if (i == nt) { t[GT_TI + i] = tb; ++nt; }
      t[GT_TM + i] |= 1u << j;
    }
    t[GT_NT] = nt;
    const uint32_t seed0 = (uint32_t)seeds.size();
    std::vector<uint32_t> stb;  // each seed's table
    for (uint32_t j = 0; j < sg; ++j) {  // one seed entry per distinct (origin, table); its own entry
      const uint32_t org = origins[s0 + j], tb = stab ? stab[s0 + j] : 0u;
      size_t i = seed0;
      while (i < seeds.size() && ((seeds[i].x & 0xFFFFFFu) != org || stb[i - seed0] != tb)) ++i;
      if (i == seeds.size()) {
        seeds.push_back(MvSeed{org | ((uint32_t)bucket[org] << 24), 0u});
        stb.push_back(tb);
      }
      seeds[i].y |= 1u << j;
    }
    t[GT_NSEED] = (uint32_t)seeds.size() - seed0;
    t[GT_SEED] = seed0;
    t[GT_S0] = s0;
    t[GT_SG] = sg;
    groups.push_back(MvGroup{s0, sg, seed0, t[GT_NSEED]});
  }
}

}  // namespace gs
