// gs_tree_dom.hip -- delivery dominators: per slot the dominator tree of the recorded round's push
// graph, and the stake, node and child counts over it (include/gossip_hip.h
// gs_tree_stake_enable_dominators).
//
// The first-delivery tree (gs_tree_rec.hip) says who a node FIRST hears the message from. Node v
// dominates w when every chain of pushes from the origin to w passes through v; the stake v
// dominates is what the round's push graph cannot deliver without v. The push graph is in HBM after
// a step-wise BFS: the inbound records inb[j][pair] = hop << 24 | src (j < cnt[pair], complete by
// construction), the hop bytes, and from the records tree pass the first-delivery parents pt, the
// nodes bucketed by level lst, the FIFO queue q and the level starts lv (level d is positions
// [lv[d], lv[d + 1]) of both lst and q). Behind a recorded round:
//
//   k_td_init   dom[w] = pt[w]'s parent | its hop << 24 for every reached non-origin node, NONE for
//               the rest; clears the round's counts and the sweeps' change words.
//   the sweeps  a monotone fixpoint. One lane per node w of a level takes x = dom[w] and, for every
//               recorded source y of w, replaces x by the nearest common ancestor of x and y in the
//               forest dom[] describes: two fingers, and the one with the larger (hop, id) key
//               moves up. A dominator's hop is strictly below its node's, so the keys fall along
//               every path, the fingers meet at the common ancestor, and a walk takes at most
//               2 x 253 steps. Every record counts, those from the same level and from deeper
//               sources too. Values only move towards the origin and every value ever stored is a
//               dominator-tree ancestor or a node above one, so lanes may read words other lanes
//               are rewriting: a walk over a mix of old and new words ends at a node that is still
//               above (or at) the true dominator, and the sweep that changes nothing read final
//               words only. Then dom[w] is an ancestor of every source of every w, which makes each
//               forest ancestor a dominator; it never rose above the true one, so it is the true one.
//     what a step costs   dom[] carries the HOP of the dominator in its top byte (pt's format: the
//               walk's consumers mask it), so a finger's next id and next key come from ONE 4-byte
//               load, and both fingers' ids and hops stay in registers: the walk is a chain of
//               single dependent loads, half of what reading dom[] and then hops[] would be. The hop
//               byte comes from the hops array (k_td_init, and hops[src] for a record's source),
//               never from the record's own byte. A node whose word already names hop 0 (the
//               origin) is done for good and reads no record: after the first sweep that is most of
//               a well-connected network, and later sweeps touch only the nodes still in doubt.
//     records   lanes follow lst, not q: within a level lst keeps the ids of each block of 1,024
//               nodes together (k_trr_bucket), and inb is row-major over pairs, so a wave's loads of
//               record row j fall into a few 4 KB windows instead of one line per lane as in queue
//               order. Record j + 1 is loaded before the walk for record j starts.
//     no LDS    a walk leaves the level at its first step and reaches ancestors of any level by node
//               id, so staging a level's words would serve the first load of a walk only; the words
//               are read from L2 (below).
//     k_td_wide   one launch per level whose widest slot is above 256 nodes, grid
//                 (ceil(wmax / 256), S); k_td_thin one launch per maximal run of thinner levels, one
//                 workgroup per slot, a barrier per level. Levels go shallowest first (level 1 is
//                 the origin's own pushes: nothing to do), so within a sweep a level reads the
//                 words the levels above it have just settled.
//     the loop is on the host: every sweep ORs 1 into its own word of flag[] when a lane stored,
//               the host reads that word back behind the sweep and stops at the first zero, at most
//               TDOM_MAX_SWEEPS sweeps. No workgroup waits on another.
//   the sums    launch_tstake_walk (gs_tree_stake_rec.hip) over dom[] gives below[]; the same
//               deepest-first walk here (k_tdc_wide / k_tdc_thin) gives per pair
//               kids << 32 | sub in a u64: a node may be the immediate dominator of all n - 1
//               others, so the two counts do not fit one u32 at 24 bits each. Adjacent lanes with
//               the same dominator (most of a level names the origin) are summed in the wave by a
//               segmented scan and issue one atomic. Then k_tstake_reduce<32, u64> and
//               k_tstake_fold of gs_tree_stake.hip.
// Launches per recorded round, L1 = (wide levels) + (runs of thin levels) over levels 1.., L2 the
// same over levels 2..: 1 + sweeps x L2 + 2 x L1 + 2.
//
// Stale lines: k_td_thin reads words the same launch wrote one level (or one lane) earlier, so it
// loads dom[] with relaxed agent-scope atomic loads (served by L2, never by a CU's L1), stores with
// agent-scope atomic stores, and every wave passes an agent-scope release fence before the level's
// barrier -- the discipline gs_tree_stake_rec.hip's header explains. A stale word would only be an
// older valid one. The wide kernels read plainly: what they need was written by earlier launches.
//
// Out-of-range input changes values only (gs_tree_stake_rec.hip's clamps): level bounds are clamped
// to N, a list or queue entry >= N is skipped, a source >= N or without a hop is skipped, a word
// that names no node or whose hop does not fall ends that record's walk without a change.
#include <algorithm>

#include "gs_device.h"
#include "gs_internal.h"

namespace gs {

namespace {

typedef unsigned long long u64;

constexpr uint32_t TD_B = 256;  // block width: the thin / wide threshold and the wide kernels' tile
constexpr uint32_t TD_NONE = 0xFFFFFFFFu;
constexpr uint32_t TD_ID = 0xFFFFFFu;
constexpr uint32_t TD_IT = 4;   // pairs per thread of the init

struct TdArgs {
  const uint32_t* lst;   // [PAIRS] nodes by level
  const uint32_t* q;     // [PAIRS] the FIFO queue
  const uint32_t* lv;    // [S][lvs] level starts
  const uint32_t* pt;    // [PAIRS] first-delivery parent | take << 24
  const uint8_t* hops;   // [PAIRS]
  const uint32_t* cnt;   // [PAIRS] in-degrees
  const uint32_t* inb;   // [capin][PAIRS] records
  uint32_t* dom;         // [PAIRS] immediate dominator | its hop << 24
  u64* ks;               // [PAIRS] kids << 32 | sub
  uint32_t* flag;        // [TDOM_MAX_SWEEPS]
  size_t PAIRS;
  uint32_t N, lvs, capin;
};

__global__ __launch_bounds__(TD_B) void k_td_init(TdArgs a) {
  const size_t base = (size_t)blockIdx.y * a.N;
  if (blockIdx.x == 0 && blockIdx.y == 0)
    for (uint32_t k = threadIdx.x; k < TDOM_MAX_SWEEPS; k += TD_B) a.flag[k] = 0;
#pragma unroll
  for (uint32_t k = 0; k < TD_IT; ++k) {
    const uint32_t v = blockIdx.x * (TD_B * TD_IT) + k * TD_B + threadIdx.x;
    if (v >= a.N) break;
    const uint32_t h = a.hops[base + v], x = a.pt[base + v], par = x & TD_ID;
    uint32_t word = TD_NONE;
    if (h >= 1 && h <= 253 && x != TD_NONE && par < a.N) {  // (pt of a node this round did not reach is stale)
      const uint32_t hp = a.hops[base + par];
      if (hp < h) word = par | hp << 24;
    }
    a.dom[base + v] = word;
    a.ks[base + v] = 0;
  }
}

template <bool AL>
__device__ inline uint32_t td_load(const uint32_t* dom, uint32_t v) {
  return AL ? __hip_atomic_load(&dom[v], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : dom[v];
}

// List position i of slot o (i < hi: the lane has one). AL: words of other nodes may have been
// stored by this launch (see the header). Returns whether dom[w] moved.
template <bool AL>
__device__ inline bool td_visit(const TdArgs& a, uint32_t o, uint32_t i, uint32_t hi) {
  if (i >= hi) return false;
  const size_t base = (size_t)o * a.N;
  const uint32_t w = a.lst[base + i];
  if (w >= a.N) return false;
  uint32_t* dom = a.dom + base;
  const uint8_t* hops = a.hops + base;
  const uint32_t cur = dom[w];  // (its own word: no other lane stores it)
  uint32_t x = cur & TD_ID, hx = cur >> 24;
  if (cur == TD_NONE || x >= a.N || hx == 0) return false;  // (hop 0: the origin, final)
  const size_t p = base + w;
  const uint32_t c = min(a.cnt[p], a.capin);
  uint32_t next = c ? a.inb[p] : 0u;
  for (uint32_t j = 0; j < c && hx; ++j) {
    const uint32_t r = next;
    if (j + 1 < c) next = a.inb[(size_t)(j + 1) * a.PAIRS + p];
    uint32_t y = r & TD_ID;
    if (y >= a.N) continue;
    uint32_t hy = hops[y];
    if (hy > 253) continue;  // (no hop: the source was not reached)
    uint32_t fx = x, fh = hx;
    bool met = true;
    while (fx != y) {  // the finger with the larger (hop, id) moves up; its hop falls at every step
      const bool mx = fh > hy || (fh == hy && fx > y);
      const uint32_t nw = td_load<AL>(dom, mx ? fx : y);
      const uint32_t ni = nw & TD_ID, nh = nw >> 24;
      if (nw == TD_NONE || ni >= a.N || nh >= (mx ? fh : hy)) { met = false; break; }
      if (mx) { fx = ni; fh = nh; }
      else { y = ni; hy = nh; }
    }
    if (met) { x = fx; hx = fh; }
  }
  if (x == (cur & TD_ID)) return false;
  const uint32_t word = x | hx << 24;
  if (AL) __hip_atomic_store(&dom[w], word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else dom[w] = word;
  return true;
}

// one OR per wave that moved a word
__device__ inline void td_report(uint32_t* flag, bool moved) {
  if (__ballot(moved) && (threadIdx.x & 63u) == 0) atomicOr(flag, 1u);
}

// Level dd of every slot: grid (ceil(widest slot / 256), S).
__global__ __launch_bounds__(TD_B) void k_td_wide(TdArgs a, uint32_t dd, uint32_t sweep) {
  const uint32_t o = blockIdx.y;
  const uint32_t* l = a.lv + (size_t)o * a.lvs;
  const uint32_t lo = min(l[dd], a.N), hi = min(l[dd + 1], a.N);
  if (lo + blockIdx.x * TD_B >= hi) return;  // (block-uniform)
  td_report(a.flag + sweep, td_visit<false>(a, o, lo + blockIdx.x * TD_B + threadIdx.x, hi));
}

// Levels d_lo up to d_hi of one slot per workgroup (2 <= d_lo <= d_hi <= 253).
__global__ __launch_bounds__(TD_B) void k_td_thin(TdArgs a, uint32_t d_lo, uint32_t d_hi, uint32_t sweep) {
  const uint32_t o = blockIdx.x;
  const uint32_t* l = a.lv + (size_t)o * a.lvs;
  bool moved = false;
  for (uint32_t dd = max(d_lo, 1u); dd <= min(d_hi, 253u); ++dd) {
    const uint32_t lo = min(l[dd], a.N), hi = min(l[dd + 1], a.N);
    for (uint32_t i0 = lo; i0 < hi; i0 += TD_B)  // (block-uniform)
      moved |= td_visit<true>(a, o, i0 + threadIdx.x, hi);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __syncthreads();
  }
  td_report(a.flag + sweep, moved);
}

// One queue position per lane (every lane of the wave calls this): w adds 1 child and sub[w] + 1
// dominated nodes to its immediate dominator; runs of equal dominators are summed in the wave.
// AL: ks[w] may have been added to by this launch.
template <bool AL>
__device__ inline void td_count(const TdArgs& a, uint32_t o, uint32_t i, uint32_t hi) {
  const size_t base = (size_t)o * a.N;
  u64* ks = a.ks + base;
  uint32_t p = TD_NONE;
  u64 val = 0;
  if (i < hi) {
    const uint32_t w = a.q[base + i];
    if (w < a.N) {
      const uint32_t x = a.dom[base + w];
      if (x != TD_NONE && (x & TD_ID) < a.N) {
        p = x & TD_ID;
        const u64 own = AL ? __hip_atomic_load(&ks[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : ks[w];
        val = 1ull << 32 | ((uint32_t)own + 1u);
      }
    }
  }
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t before = __shfl_up(p, 1, 64);
  const u64 heads = __ballot(lane == 0 || before != p);
  const uint32_t start = 63u - (uint32_t)__clzll(heads & (~0ull >> (63u - lane)));  // (lane 0 is a head)
#pragma unroll
  for (uint32_t s = 1; s < 64; s <<= 1) {
    const uint32_t ul = __shfl_up((uint32_t)val, s, 64), uh = __shfl_up((uint32_t)(val >> 32), s, 64);
    if (lane >= start + s) val += (u64)uh << 32 | ul;  // (both halves stay below 2^24: no carry between them)
  }
  const bool last = lane == 63 || (heads >> (lane + 1) & 1ull);
  if (last && p != TD_NONE) atomicAdd(&ks[p], val);
}

__global__ __launch_bounds__(TD_B) void k_tdc_wide(TdArgs a, uint32_t dd) {
  const uint32_t o = blockIdx.y;
  const uint32_t* l = a.lv + (size_t)o * a.lvs;
  const uint32_t lo = min(l[dd], a.N), hi = min(l[dd + 1], a.N);
  if (lo + blockIdx.x * TD_B >= hi) return;  // (block-uniform)
  td_count<false>(a, o, lo + blockIdx.x * TD_B + threadIdx.x, hi);
}

// Levels d_hi down to d_lo of one slot per workgroup (1 <= d_lo <= d_hi <= 253).
__global__ __launch_bounds__(TD_B) void k_tdc_thin(TdArgs a, uint32_t d_lo, uint32_t d_hi) {
  const uint32_t o = blockIdx.x;
  const uint32_t* l = a.lv + (size_t)o * a.lvs;
  for (uint32_t dd = min(d_hi, 253u); dd >= max(d_lo, 1u); --dd) {
    const uint32_t lo = min(l[dd], a.N), hi = min(l[dd + 1], a.N);
    for (uint32_t i0 = lo; i0 < hi; i0 += TD_B)  // (block-uniform)
      td_count<true>(a, o, i0 + threadIdx.x, hi);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __syncthreads();
  }
}

}  // namespace

hipError_t launch_tstake_dom(Engine& e, bool* capped) {
  *capped = false;
  if (!e.trr_q || !e.trr_lst || !e.trr_pt || !e.trr_hmeta || !e.inb || !e.cnt || !e.ts_idom || !e.ts_ks || !e.ts_flag ||
      !e.ts_hflag || e.PAIRS != (size_t)e.S * e.N)
    return hipErrorInvalidValue;
  TdArgs a;
  a.lst = e.trr_lst; a.q = e.trr_q; a.lv = e.trr_lv; a.pt = e.trr_pt; a.hops = e.hops; a.cnt = e.cnt; a.inb = e.inb;
  a.dom = e.ts_idom; a.ks = reinterpret_cast<u64*>(e.ts_ks); a.flag = e.ts_flag;
  a.PAIRS = e.PAIRS; a.N = e.N; a.lvs = (uint32_t)(tree_rec_lv_words(e) / e.S); a.capin = e.capin;
  const uint32_t maxd = std::min(e.trr_hmeta[0], 253u);
  const uint32_t* wmax = e.trr_hmeta + 1;
  const dim3 blk(TD_B);
  auto wide = [&](uint32_t d) { return dim3((wmax[d] + TD_B - 1) / TD_B, e.S); };
  hipEvent_t t0;
  hipError_t r;
  e.tbegin("tree_stake", &t0);
  hipLaunchKernelGGL(k_td_init, dim3((e.N + TD_B * TD_IT - 1) / (TD_B * TD_IT), e.S), blk, 0, e.st, a);
  r = hipGetLastError();
  e.tend("tree_stake", t0);
  if (r != hipSuccess) return r;

  uint32_t sweeps = 0;
  while (maxd >= 2) {
    if (sweeps == TDOM_MAX_SWEEPS) { *capped = true; return hipSuccess; }
    for (uint32_t dd = 2; dd <= maxd;) {  // shallowest first
      if (!wmax[dd]) { ++dd; continue; }
      e.tbegin("tree_stake", &t0);
      if (wmax[dd] > TD_B) {
        hipLaunchKernelGGL(k_td_wide, wide(dd), blk, 0, e.st, a, dd, sweeps);
        ++dd;
      } else {
        uint32_t d_hi = dd;
        while (d_hi < maxd && wmax[d_hi + 1] <= TD_B) ++d_hi;
        hipLaunchKernelGGL(k_td_thin, dim3(e.S), blk, 0, e.st, a, dd, d_hi, sweeps);
        dd = d_hi + 1;
      }
      r = hipGetLastError();
      e.tend("tree_stake", t0);
      if (r != hipSuccess) return r;
    }
    r = hipMemcpyAsync(e.ts_hflag, e.ts_flag + sweeps, 4, hipMemcpyDeviceToHost, e.st);
    if (r == hipSuccess) r = hipStreamSynchronize(e.st);
    if (r != hipSuccess) return r;
    ++sweeps;
    if (!*e.ts_hflag) break;
  }
  e.ts_sweeps = sweeps;

  r = launch_tstake_walk(e, e.ts_idom);  // below[] over the dominator tree
  if (r != hipSuccess) return r;
  for (uint32_t dd = maxd; dd >= 1;) {  // kids and sub, deepest first
    if (!wmax[dd]) { --dd; continue; }
    e.tbegin("tree_stake", &t0);
    if (wmax[dd] > TD_B) {
      hipLaunchKernelGGL(k_tdc_wide, wide(dd), blk, 0, e.st, a, dd);
      --dd;
    } else {
      uint32_t d_lo = dd;
      while (d_lo > 1 && wmax[d_lo - 1] <= TD_B) --d_lo;
      hipLaunchKernelGGL(k_tdc_thin, dim3(e.S), blk, 0, e.st, a, d_lo, dd);
      dd = d_lo - 1;
    }
    r = hipGetLastError();
    e.tend("tree_stake", t0);
    if (r != hipSuccess) return r;
  }
  return hipSuccess;
}

}  // namespace gs
