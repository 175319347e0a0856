// gs_tree_stake_rec.hip -- the delivery tree in stake at any node count: a level walk over what
// the records tree pass (gs_tree_rec.hip) leaves in HBM (include/gossip_hip.h
// gs_tree_stake_enable_records).
//
// k_tstake_up (gs_tree_stake.hip) keeps a slot's whole tree in one workgroup's LDS and stops at
// 10,175 nodes. Here nothing is sorted and nothing is kept on-chip: until the next recorded round
// the records pass holds per slot the FIFO queue q (level d is q[lv[d], lv[d + 1])), per node
// pt = parent | take index << 24, the child bits cmask and the round's subtree sizes ex, and on the
// host the deepest level and each level's widest slot (Engine::trr_hmeta, read back by that pass:
// no host wait here). Behind a recorded round:
//
//   the walk   below[] (u64 per pair) is cleared by a memset, then the levels go deepest first: a
//              node w of level dd adds below[w] + stake[w] to below[parent(w)], in place. Its own
//              value is final (its children were the step before), so there is no second array and
//              no final subtraction. A level is read in QUEUE order, one lane per queue position:
//              the order within a level is (queue position of the parent, take index), so the
//              children of one parent sit in adjacent lanes. The wave runs a segmented inclusive
//              scan of its 64 u64 values over those runs (head flags from one ballot, __shfl_up on
//              both halves) and only a run's last lane issues the u64 atomicAdd: in the levels
//              where every node has `fanout` children that is 1 / fanout of the atomics. A run cut
//              by a wave or block edge becomes two atomics. The head flags compare neighbours
//              only, so parents that are not grouped (out-of-range input) cost atomics, not sums.
//     k_tsr_wide   one launch per level whose widest slot is above 256 nodes, grid
//                  (ceil(wmax / 256), S) as k_trr_up's. Levels are separated by launches: no grid
//                  barrier, no spin-wait.
//     k_tsr_thin   one launch per maximal run of consecutive levels of at most 256 nodes: one
//                  256-thread workgroup per slot walks the run's levels deepest first with a
//                  barrier between them, so a BFS's head and tail (and the whole 253-level chain)
//                  cost one launch and not one per level.
//   k_tsr_pack ks = popc(cmask) << 24 | ex per pair, coalesced: the round's child count (at most
//              32) and subtree size (below 2^24 = GS_MAX_NODES + 1) the tree pass already holds.
//   then k_tstake_reduce<24> and k_tstake_fold of gs_tree_stake.hip.
// Launches per recorded round: (wide levels) + (runs of thin levels) + 3.
//
// The stale-line question of k_tsr_thin. The adds are device-scope atomics and are performed in
// L2; a plain load of below[w] one level later could be served from the CU's L1, which an atomic
// of another wave does not update (a line fetched for a neighbouring node of an earlier level
// would still hold the old value). So below[w] is read with a relaxed agent-scope atomic load,
// which is served by L2 and never by L1, and every wave passes an agent-scope release fence (its
// atomics have been performed) before the barrier that ends the level. Nothing else the kernel
// reads is written while it runs (q, pt, lv, stake), and no L1 invalidate is needed. k_tsr_wide
// reads below[w] plainly: the adds it reads were made by an earlier launch.
//
// Out-of-range input (after a round that raised the 253-hop error, or one whose place pass raised
// the bounds error, q may hold the previous round's entries) changes values only: level bounds are
// clamped to N, a queue entry >= N is skipped, a parent >= N is no parent, the level loop ends at
// 253 (lv has 257 entries per slot).
#include <algorithm>

#include "gs_device.h"
#include "gs_internal.h"

namespace gs {

namespace {

typedef unsigned long long u64;

constexpr uint32_t TSR_B = 256;           // block width: the thin / wide threshold and the wide kernel's tile
constexpr uint32_t TSR_NONE = 0xFFFFFFFFu;
constexpr uint32_t TSR_IT = 4;            // pairs per thread of the pack

// One queue position per lane (i < hi: the lane has one; every lane of the wave calls this).
// AL: below[w] may have been added to by this launch (see the header).
template <bool AL>
__device__ inline void tsr_step(const uint32_t* __restrict__ q, const uint32_t* __restrict__ pt,
                                const uint64_t* __restrict__ stake, u64* below, uint32_t N, uint32_t i, uint32_t hi) {
  uint32_t p = TSR_NONE;
  u64 val = 0;
  if (i < hi) {
    const uint32_t w = q[i];
    if (w < N) {
      const uint32_t x = pt[w];
      if (x != TSR_NONE && (x & 0xFFFFFFu) < N) {
        p = x & 0xFFFFFFu;
        val = (AL ? __hip_atomic_load(&below[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : below[w]) + stake[w];
      }
    }
  }
  // segmented inclusive scan over the runs of equal parents: a run starts where the lane before has another
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t before = __shfl_up(p, 1, 64);
  const u64 heads = __ballot(lane == 0 || before != p);
  const uint32_t start = 63u - (uint32_t)__clzll(heads & (~0ull >> (63u - lane)));  // (lane 0 is a head)
#pragma unroll
  for (uint32_t o = 1; o < 64; o <<= 1) {
    const uint32_t ul = __shfl_up((uint32_t)val, o, 64), uh = __shfl_up((uint32_t)(val >> 32), o, 64);
    if (lane >= start + o) val += (u64)uh << 32 | ul;
  }
  const bool last = lane == 63 || (heads >> (lane + 1) & 1ull);
  if (last && p != TSR_NONE && val) atomicAdd(&below[p], val);
}

// Level dd of every slot: grid (ceil(widest slot / 256), S).
__global__ __launch_bounds__(TSR_B) void k_tsr_wide(const uint32_t* __restrict__ q, const uint32_t* __restrict__ pt,
                                                    const uint32_t* __restrict__ lv, const uint64_t* __restrict__ stake,
                                                    u64* below, uint32_t N, uint32_t lvs, uint32_t dd) {
  const uint32_t o = blockIdx.y;
  const uint32_t* l = lv + (size_t)o * lvs;
  const uint32_t lo = min(l[dd], N), hi = min(l[dd + 1], N);
  if (lo + blockIdx.x * TSR_B >= hi) return;  // (block-uniform)
  const size_t base = (size_t)o * N;
  tsr_step<false>(q + base, pt + base, stake, below + base, N, lo + blockIdx.x * TSR_B + threadIdx.x, hi);
}

// Levels d_hi down to d_lo of one slot per workgroup (1 <= d_lo <= d_hi <= 253, each at most 256
// wide in every slot; a wider one would only take more trips).
__global__ __launch_bounds__(TSR_B) void k_tsr_thin(const uint32_t* __restrict__ q, const uint32_t* __restrict__ pt,
                                                    const uint32_t* __restrict__ lv, const uint64_t* __restrict__ stake,
                                                    u64* below, uint32_t N, uint32_t lvs, uint32_t d_lo,
                                                    uint32_t d_hi) {
  const uint32_t o = blockIdx.x;
  const uint32_t* l = lv + (size_t)o * lvs;
  const size_t base = (size_t)o * N;
  for (uint32_t dd = min(d_hi, 253u); dd >= max(d_lo, 1u); --dd) {
    const uint32_t lo = min(l[dd], N), hi = min(l[dd + 1], N);
    for (uint32_t i0 = lo; i0 < hi; i0 += TSR_B)  // (block-uniform)
      tsr_step<true>(q + base, pt + base, stake, below + base, N, i0 + threadIdx.x, hi);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __syncthreads();
  }
}

__global__ __launch_bounds__(TSR_B) void k_tsr_pack(const uint32_t* __restrict__ cmask, const uint32_t* __restrict__ ex,
                                                    uint32_t* __restrict__ ks, size_t pairs) {
#pragma unroll
  for (uint32_t k = 0; k < TSR_IT; ++k) {
    const size_t p = (size_t)blockIdx.x * (TSR_B * TSR_IT) + k * TSR_B + threadIdx.x;
    if (p >= pairs) break;
    ks[p] = (uint32_t)__popc(cmask[p]) << 24 | (ex[p] & 0xFFFFFFu);
  }
}

}  // namespace

// The walk behind a recorded round whose records tree pass ran, over the tree whose parents are pt
// (the pass's own, or the dominator kind's: gs_tree_dom.hip), each launch timed as one of
// "tree_stake". e.trr_hmeta is still this round's.
hipError_t launch_tstake_walk(Engine& e, const uint32_t* pt) {
  if (!e.trr_q || !e.trr_hmeta || !e.ts_below || !pt || e.PAIRS != (size_t)e.S * e.N) return hipErrorInvalidValue;
  u64* below = reinterpret_cast<u64*>(e.ts_below);
  hipError_t r = hipMemsetAsync(below, 0, e.PAIRS * 8, e.st);
  if (r != hipSuccess) return r;
  const uint32_t maxd = std::min(e.trr_hmeta[0], 253u);
  const uint32_t* wmax = e.trr_hmeta + 1;
  const uint32_t lvs = (uint32_t)(tree_rec_lv_words(e) / e.S);  // per-slot stride of the level starts
  hipEvent_t t0;
  for (uint32_t dd = maxd; dd >= 1;) {
    if (!wmax[dd]) { --dd; continue; }  // (no slot has the level)
    e.tbegin("tree_stake", &t0);
    if (wmax[dd] > TSR_B) {
      k_tsr_wide<<<dim3((wmax[dd] + TSR_B - 1) / TSR_B, e.S), TSR_B, 0, e.st>>>(e.trr_q, pt, e.trr_lv, e.stake, below, e.N,
                                                                              lvs, dd);
      --dd;
    } else {
      uint32_t d_lo = dd;
      while (d_lo > 1 && wmax[d_lo - 1] <= TSR_B) --d_lo;  // (an empty level walks nothing)
      k_tsr_thin<<<e.S, TSR_B, 0, e.st>>>(e.trr_q, pt, e.trr_lv, e.stake, below, e.N, lvs, d_lo, dd);
      dd = d_lo - 1;
    }
    r = hipGetLastError();
    e.tend("tree_stake", t0);
    if (r != hipSuccess) return r;
  }
  return hipSuccess;
}

// The records mode's walk and pack (Engine::ts_rec); launch_tstake_reduce and launch_tstake_fold
// follow.
hipError_t launch_tstake_rec(Engine& e) {
  hipError_t r = launch_tstake_walk(e, e.trr_pt);
  if (r != hipSuccess) return r;
  hipEvent_t t0;
  e.tbegin("tree_stake", &t0);
  k_tsr_pack<<<(uint32_t)((e.PAIRS + TSR_B * TSR_IT - 1) / (TSR_B * TSR_IT)), TSR_B, 0, e.st>>>(e.trr_cmask, e.trr_ex,
                                                                                             e.ts_ks, e.PAIRS);
  r = hipGetLastError();
  e.tend("tree_stake", t0);
  return r;
}

}  // namespace gs
