// gs_reach.hip -- the stake reach view: nodes and stake reached per hop, summed over the slots
// of a group (include/gossip_hip.h gs_reach_*).
//
// After a recorded round's last kernel, two launches on the engine's stream read the hop bytes
// the round left -- exactly what gs_read_hops returns per slot -- and the per-node stakes:
//
//   k_reach_reduce  per group g and hop byte b, into u64 scratch [G][256][3]:
//                     sum_j w_j #{v : h_j[v] == b},  sum w_j lo32(stake[v]),  sum w_j hi32(stake[v])
//                   over the group's slots j and the nodes v with h_j[v] == b. Grid (node blocks,
//                   chunks of gs_cluster_plan.h: a chunk lies in one group). A lane owns four
//                   consecutive nodes and keeps their stakes as 32-bit limbs in registers for
//                   every slot of the chunk; a wave covers 256 nodes and the block's four waves
//                   split the chunk's slots, so a slot's weight is uniform over the wave. Per
//                   slot a lane loads one u32 of four hop bytes (bytes where slot * NP + v0 is no
//                   multiple of 4 or NP cuts the node group).
//                   In a gossip BFS nearly every node of a slot sits in three or four hop bins,
//                   so a shared histogram would serialise on its LDS atomics. Hops below RC_FB
//                   go to lane-private LDS columns [wave][RC_FB][3][64 lanes] u64 instead: the
//                   bank is the lane, a lane touches only its own column, no atomics. Hops from
//                   RC_FB on (deep graphs, and 255: unreached) go to one per-block histogram
//                   [256][3] with LDS atomics. At the end each wave sums its columns over the
//                   lanes (shuffles) into the block histogram, and the block adds the non-zero
//                   (bin, word) sums to the group's scratch: one no-return u64 atomicAdd each.
//   k_reach_fold    one thread per (group, bin), no atomics: scratch -> the round's 128-bit stake
//                   lo_sum + (hi_sum << 32) and its node count, stored as the last round's values
//                   and added to the totals with carry; scratch zeroed for the next round.
//
// LDS: 4 waves x RC_FB x 3 x 64 x 8 B = 49,152 B of private columns + 6,144 B of histogram =
// 55,296 B a block with RC_FB = 8: static (below 64 KB), and two blocks fit a compute unit's
// 160 KB. Limbs: a group's round sums are at most (sum of weights) x n_nodes x (2^32 - 1), below
// 2^64 under gs_reach_enable_groups' bound (sum of weights) x n_nodes < 2^32.
#include "gs_device.h"
#include "gs_internal.h"

namespace gs {

namespace {

typedef unsigned long long u64;

constexpr uint32_t RC_NODES = 256;  // nodes per block (64 lanes x 4)
constexpr uint32_t RC_FB = 8;       // hop bins kept in lane-private columns
constexpr uint32_t RC_WORDS = 3;    // weighted count, sum w lo32(stake), sum w hi32(stake)

static_assert(RC_NODES == CLUSTER_PLAN_NODES, "the chunk table is planned for the cluster view's node blocks");
static_assert(sizeof(ClusterChunk) == sizeof(uint3), "k_reach_reduce reads a chunk as a uint3");
static_assert((4 * RC_FB * 64 + 256) * RC_WORDS * sizeof(u64) <= 64 * 1024, "static LDS of k_reach_reduce");

__device__ __forceinline__ u64 rc_wave_sum(u64 x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
  return x;
}

// grid (node blocks, chunks): blockIdx.y indexes the chunk table {group, s_lo, s_hi}
__global__ __launch_bounds__(256) void k_reach_reduce(const uint8_t* __restrict__ hops,
                                                      const uint64_t* __restrict__ stake, uint32_t NP,
                                                      const uint3* __restrict__ chunks,
                                                      const uint32_t* __restrict__ wts, u64* __restrict__ scr) {
  __shared__ u64 priv[4][RC_FB][RC_WORDS][64];
  __shared__ u64 hist[256][RC_WORDS];
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // (uniform: the weights load as scalars)
  const uint32_t v0 = blockIdx.x * RC_NODES + lane * 4;
  const uint32_t nv = v0 < NP ? min(4u, NP - v0) : 0u;  // this lane's nodes in range
  const uint3 ch = chunks[blockIdx.y];
  const uint32_t per = (ch.z - ch.y + 3) / 4;
  const uint32_t s_lo = min(ch.z, ch.y + wave * per);
  const uint32_t s_hi = min(ch.z, s_lo + per);
  const bool busy = s_lo < s_hi;  // (a short chunk leaves waves without a slot: they only join the flush)
#pragma unroll
  for (uint32_t w = 0; w < RC_WORDS; ++w) hist[threadIdx.x][w] = 0;
  if (busy) {
#pragma unroll
    for (uint32_t b = 0; b < RC_FB; ++b)
#pragma unroll
      for (uint32_t w = 0; w < RC_WORDS; ++w) priv[wave][b][w][lane] = 0;
  }
  __syncthreads();
  if (busy && nv) {
    uint32_t slo[4], shi[4];
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
      const uint64_t s = k < nv ? stake[v0 + k] : 0;
      slo[k] = (uint32_t)s;
      shi[k] = (uint32_t)(s >> 32);
    }
    for (uint32_t j = s_lo; j < s_hi; ++j) {
      const uint32_t w = wts[j];
      if (!w) continue;  // (uniform: the slot is not read at all)
      const size_t p = (size_t)j * NP + v0;
      uint32_t h = 0;
      if (nv == 4 && (p & 3) == 0) {
        h = *reinterpret_cast<const uint32_t*>(hops + p);
      } else {
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k)
          if (k < nv) h |= (uint32_t)hops[p + k] << (8 * k);
      }
#pragma unroll
      for (uint32_t k = 0; k < 4; ++k) {
        if (k >= nv) break;
        const uint32_t hb = (h >> (8 * k)) & 0xFFu;
        const u64 xl = (u64)w * slo[k], xh = (u64)w * shi[k];
        if (hb < RC_FB) {
          priv[wave][hb][0][lane] += w;
          priv[wave][hb][1][lane] += xl;
          priv[wave][hb][2][lane] += xh;
        } else {
          atomicAdd(&hist[hb][0], (u64)w);
          if (xl) atomicAdd(&hist[hb][1], xl);
          if (xh) atomicAdd(&hist[hb][2], xh);
        }
      }
    }
  }
  if (busy) {  // the wave's columns summed over the lanes (a lane reads its own column: no barrier before)
#pragma unroll
    for (uint32_t b = 0; b < RC_FB; ++b)
#pragma unroll
      for (uint32_t w = 0; w < RC_WORDS; ++w) {
        const u64 x = rc_wave_sum(priv[wave][b][w][lane]);
        if (lane == 0 && x) atomicAdd(&hist[b][w], x);
      }
  }
  __syncthreads();
  u64* gscr = scr + ((size_t)ch.x * 256 + threadIdx.x) * RC_WORDS;
#pragma unroll
  for (uint32_t w = 0; w < RC_WORDS; ++w) {
    const u64 x = hist[threadIdx.x][w];
    if (x) atomicAdd(&gscr[w], x);
  }
}

// One block per group, one thread per bin. acc: the group's [6][256] u64 -- nodes, stake lo,
// stake hi over the recorded rounds, then the same three of the last recorded round.
__global__ __launch_bounds__(256) void k_reach_fold(u64* __restrict__ scr, u64* __restrict__ acc) {
  const uint32_t b = threadIdx.x;
  u64* s = scr + ((size_t)blockIdx.x * 256 + b) * RC_WORDS;
  u64* a = acc + (size_t)blockIdx.x * 6 * 256 + b;
  const u64 c = s[0], lo = s[1], hi = s[2];
  s[0] = 0; s[1] = 0; s[2] = 0;
  const u64 rl = lo + (hi << 32);
  const u64 rh = (hi >> 32) + (rl < lo ? 1u : 0u);
  a[3 * 256] = c;
  a[4 * 256] = rl;
  a[5 * 256] = rh;
  a[0] += c;
  const u64 tl = a[1 * 256] + rl;
  a[1 * 256] = tl;
  a[2 * 256] += rh + (tl < rl ? 1u : 0u);
}

}  // namespace

// The recorded round's reduction and fold (Engine::rc_on; the scratch is zero between rounds).
hipError_t launch_reach_reduce(Engine& e) {
  const dim3 grid((e.NP + RC_NODES - 1) / RC_NODES, e.rc_nchunks);
  k_reach_reduce<<<grid, 256, 0, e.st>>>(e.hops, e.stake, e.NP, reinterpret_cast<const uint3*>(e.rc_chunks), e.rc_wts,
                                         reinterpret_cast<u64*>(e.rc_scr));
  return hipGetLastError();
}

hipError_t launch_reach_fold(Engine& e) {
  k_reach_fold<<<e.rc_G, 256, 0, e.st>>>(reinterpret_cast<u64*>(e.rc_scr), reinterpret_cast<u64*>(e.rc_acc));
  return hipGetLastError();
}

}  // namespace gs
