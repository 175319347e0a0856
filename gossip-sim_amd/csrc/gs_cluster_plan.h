// gs_cluster_plan.h -- slot chunks of the grouped cluster load view (plain C++, no device code:
// gs_engine.hip builds the table at gs_cluster_enable_groups and tests/cluster_plan_check.cpp
// checks it stand-alone).
//
// The grouped reduction (gs_cluster.hip, k_cluster_reduce_g) sums the slots of one group into
// that group's scratch, so a block's slots must lie in one group. blockIdx.y indexes this table:
// one entry per chunk {group, s_lo, s_hi}, the chunks of a group tiling [a_g, a_g + n_g) in slot
// order with `chunk` slots each (the last one what is left).
//
// `chunk` is what the ungrouped view uses (cluster_chunk_slots): with nb node blocks of 256
// nodes, want = ceil(2,048 / nb) chunks would give about 2,048 blocks, so chunk = ceil(S / want)
// rounded up to 16. A group adds at most one short chunk:
//     G <= chunks <= floor(S / chunk) + G <= want + G.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace gs {

struct ClusterChunk { uint32_t group, s_lo, s_hi; };  // slots [s_lo, s_hi) of group `group`

constexpr uint32_t CLUSTER_PLAN_NODES = 256;    // nodes per block of the reduction
constexpr uint32_t CLUSTER_PLAN_BLOCKS = 2048;  // blocks aimed for (~8 per compute unit)

// chunks the plan aims for at NP nodes (the bound above is in terms of it)
inline uint32_t cluster_plan_want(uint32_t NP) {
  const uint32_t nb = (uint32_t)(((uint64_t)NP + CLUSTER_PLAN_NODES - 1) / CLUSTER_PLAN_NODES);
  return std::max(1u, (CLUSTER_PLAN_BLOCKS + std::max(1u, nb) - 1) / std::max(1u, nb));
}

// slots per full chunk: a multiple of 16 (a wave takes a quarter of a chunk)
inline uint32_t cluster_plan_chunk(uint32_t NP, uint32_t S) {
  const uint32_t want = cluster_plan_want(NP);
  const uint32_t per = (uint32_t)(((uint64_t)S + want - 1) / want);
  return std::max(16u, (per + 15u) & ~15u);
}

// The chunk table of groups of `sizes[g]` consecutive slots (every size >= 1).
inline std::vector<ClusterChunk> cluster_plan_build(uint32_t NP, const uint32_t* sizes, uint32_t n_groups) {
  uint64_t S = 0;
  for (uint32_t g = 0; g < n_groups; ++g) S += sizes[g];
  const uint32_t chunk = cluster_plan_chunk(NP, (uint32_t)S);
  std::vector<ClusterChunk> out;
  uint32_t a = 0;
  for (uint32_t g = 0; g < n_groups; ++g) {
    const uint32_t end = a + sizes[g];
    for (uint32_t lo = a; lo < end; lo += chunk) out.push_back(ClusterChunk{g, lo, std::min(end, lo + chunk)});
    a = end;
  }
  return out;
}

}  // namespace gs
