// gs_tree_wg.hip -- the delivery tree of one origin slot inside one workgroup.
//
// Cluster::mst (gossip.rs:580-591) is the tree of first deliveries: parent[w] = the node that
// discovered w first in run_gossip's FIFO queue order (gossip.rs:494-615). The round kernel's
// BFS fills its level queue by LDS atomics, so its order inside a level is arbitrary: it
// gives hops, never parents. k_tree_wg walks the same rows, prune masks, failed ranks and
// fanouts in the reference's order:
//   - the frontier of level d is q[start, start + qn) in FIFO order; thread i takes queue
//     position i (a level larger than the workgroup takes several trips, in order);
//   - claim: the lane takes its node's pushes in get_nodes(..).take(fanout) order (take index
//     t) and sends atomicMin(key[w], i << 6 | t) to every peer w still unreached;
//   - win: after a barrier the push whose key stayed in key[w] is w's first discovery:
//     parent[w], hop[w] and the lane's own child count are plain stores;
//   - place: the winners enter the next level in (i, t) order -- a lane's offset is the sum
//     over the push columns of mbcnt(ballot(column)), the waves' totals go through LDS and a
//     running base carries across trips. No sort, no inbound records.
// Subtree sizes come from walking the queue backwards one level at a time. The kernel reads
// global rows and masks and writes only its slot's three output arrays.
#include <type_traits>

#include "gs_device.h"
#include "gs_internal.h"
#include "gs_round_args.h"

namespace gs {

constexpr uint32_t TWG_THREADS = 512;  // 8 waves: a level's cross-wave prefix is 8 LDS words
constexpr uint32_t TWG_WAVES = TWG_THREADS / 64;
constexpr uint32_t TWG_IN = 4;         // nodes per trip of the setup loop (their loads issued together)
constexpr uint32_t TWG_LEVELS = 256;   // level starts: levels 0..254 and the queue's end

struct TreeOut {
  uint32_t* parent;    // [PAIRS] this round's parents
  uint32_t* kids_acc;  // [PAIRS] += first deliveries made
  uint32_t* sub_acc;   // [PAIRS] += nodes below
};

// LDS carve-up (byte offsets), shared by the host's size query and the kernel:
// 12 B per node and the prune mask (2 B while the ring has <= 16 slots, else 4 B).
struct TwgLayout {
  uint32_t wtot, lvl, key, mk, nl, q, par, hop, kids, total;
};
__host__ __device__ inline TwgLayout twg_layout(uint32_t N, uint32_t pmw) {
  TwgLayout L;
  uint32_t o = 0;
  L.wtot = o; o += 16 * 4;                 // the waves' winner counts of a trip
  L.lvl = o;  o += TWG_LEVELS * 4;         // queue position where each level starts
  L.key = o;  o += 4 * N;                  // claim keys; after the BFS the subtree sizes
  L.mk = o;   o += (pmw * N + 3) & ~3u;    // the slot's prune masks (pending rotation clear applied)
  L.nl = o;   o += (2 * N + 3) & ~3u;      // per node: ring head | len << 5 | entry bucket << 11
  L.q = o;    o += (2 * N + 3) & ~3u;      // the FIFO queue u16[N]: levels are consecutive ranges
  L.par = o;  o += (2 * N + 3) & ~3u;      // first discoverer u16
  L.hop = o;  o += (N + 3) & ~3u;
  L.kids = o; o += (N + 3) & ~3u;          // first deliveries made (<= the ring size)
  L.total = o;
  return L;
}

size_t tree_wg_lds_bytes(uint32_t N, uint32_t ASZP) { return twg_layout(N, ASZP <= 16 ? 2 : 4).total; }

// LDS bytes per node, from the layout (4,096 nodes: no array is padded)
uint32_t tree_wg_node_bytes(uint32_t ASZP) {
  return (uint32_t)((tree_wg_lds_bytes(4096, ASZP) - tree_wg_lds_bytes(0, ASZP)) / 4096);
}

// Largest N the kernel serves: the layout fits one workgroup's LDS and node ids fit u16.
uint32_t tree_wg_max_nodes(uint32_t ASZP) {
  uint32_t lo = 0, hi = 65535;
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1) / 2;
    if (tree_wg_lds_bytes(mid, ASZP) <= TREE_LDS_MAX) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// The pushed peers of a row in take order: dst[t] = peer of the t-th taken ring slot counted
// from the ring's head (the rest 0); returns their number. `pm` holds physical ring slots.
template <int ASZP, int FP>
__device__ inline uint32_t take_order(const uint32_t (&row)[ASZP], uint32_t pm, uint32_t head, uint32_t (&dst)[FP]) {
#pragma unroll
  for (int t = 0; t < FP; ++t) dst[t] = 0;
  const uint32_t below_head = (1u << head) - 1u;
  const uint32_t nhi = (uint32_t)__popc(pm & ~below_head);  // taken slots from the head to the ring's end
#pragma unroll
  for (int s = 0; s < ASZP; ++s) {
    const uint32_t lower = pm & ((1u << s) - 1u);
    const uint32_t rank = (uint32_t)s >= head ? (uint32_t)__popc(lower & ~below_head) : nhi + (uint32_t)__popc(lower);
    const bool b = (pm >> s) & 1u;
#pragma unroll
    for (int t = 0; t < FP; ++t)
      if (b && rank == (uint32_t)t) dst[t] = row[s];
  }
  return (uint32_t)__popc(pm);
}

// One workgroup per slot. Per-slot fanouts (a.sfan) and trajectory tables (a.stab) are
// workgroup-uniform run-time branches here: the kernel is latency-bound on its barriers.
template <int ASZP, int FP>
__global__ __launch_bounds__(TWG_THREADS) void k_tree_wg(RoundArgs a, TreeOut out) {
  using PMT = typename std::conditional<(ASZP <= 16), uint16_t, uint32_t>::type;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t N = a.N;
  const TwgLayout L = twg_layout(N, (uint32_t)sizeof(PMT));
  uint32_t* wtot = reinterpret_cast<uint32_t*>(smem + L.wtot);
  uint32_t* lvl = reinterpret_cast<uint32_t*>(smem + L.lvl);
  uint32_t* key = reinterpret_cast<uint32_t*>(smem + L.key);
  uint32_t* sub = key;  // (the keys are dead after the BFS)
  PMT* mk_l = reinterpret_cast<PMT*>(smem + L.mk);
  uint16_t* nl_l = reinterpret_cast<uint16_t*>(smem + L.nl);
  uint16_t* q = reinterpret_cast<uint16_t*>(smem + L.q);
  uint16_t* par = reinterpret_cast<uint16_t*>(smem + L.par);
  uint8_t* hop = smem + L.hop;
  uint8_t* kids = smem + L.kids;
  const uint32_t tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;

  const uint32_t o = blockIdx.x;
  if (a.stab) {  // the slot's own table: rows, ring size, FAIL ranks, the pending clear of its last rotation
    const uint32_t t = a.stab[o];
    a.peers += t * a.t_rows; a.hl += t * a.t_ents;
    a.frank += t * a.t_frank;
    a.ASZ = a.ttab[t].asz;
    if (a.rot_count) {
      a.rot_list += (size_t)t * N; a.rot_count += 2 * t; a.rot_changed += t * a.t_ents;
    }
  }
  const uint32_t org = a.origin[o], ob = a.obkt[o], nf = a.nfail[o];
  const uint32_t fan = a.sfan ? a.sfan[o] : a.fanout;
  const size_t base = (size_t)o * N;

  // Setup, as the round kernel's: each node's mask word and the ring head / len / bucket of the
  // entry it uses for this origin (push_active_set.rs:38-52)
  for (uint32_t v0 = tid; v0 < N; v0 += TWG_IN * TWG_THREADS) {
    uint32_t bk[TWG_IN], mw[TWG_IN], hv[TWG_IN];
#pragma unroll
    for (uint32_t k = 0; k < TWG_IN; ++k) {
      const uint32_t v = v0 + k * TWG_THREADS;
      bk[k] = v < N ? min((uint32_t)a.bucket[v], ob) : 0u;
      mw[k] = v < N ? ntl(&a.mask[base + v]) : 0u;
    }
#pragma unroll
    for (uint32_t k = 0; k < TWG_IN; ++k) {
      const uint32_t v = v0 + k * TWG_THREADS;
      hv[k] = v < N ? a.hl[v * NB + bk[k]] : 0u;
    }
#pragma unroll
    for (uint32_t k = 0; k < TWG_IN; ++k) {
      const uint32_t v = v0 + k * TWG_THREADS;
      if (v >= N) break;
      hop[v] = 0xFF;
      kids[v] = 0;
      key[v] = 0xFFFFFFFFu;
      mk_l[v] = (PMT)mw[k];
      nl_l[v] = (uint16_t)((hv[k] & 0x1Fu) | ((hv[k] >> 8) << 5) | (bk[k] << 11));
    }
  }
  __syncthreads();
  if (a.rot_count) {  // the replaced ring slots of the last rotation lose this slot's prune bits
                      // (gossip.rs:739-754): in the LDS copy only, the round kernel writes them back
    const uint32_t nr = *a.rot_count;
    for (uint32_t i = tid; i < nr; i += TWG_THREADS) {
      const uint32_t u = a.rot_list[i];
      const uint32_t m = a.rot_changed[u * NB + min((uint32_t)a.bucket[u], ob)];
      if (m) mk_l[u] = (PMT)(mk_l[u] & ~m);
    }
  }
  if (tid == 0) { hop[org] = 0; q[0] = (uint16_t)org; }
  __syncthreads();

  // ---------------- ordered BFS: three barriers per level, two more per further trip --------
  uint32_t start = 0, qn = 1, d = 0;
  for (;; ++d) {
    if (qn == 0) break;
    if (d + 1 >= 255) return;  // the engine's 253-hop limit (uniform): nothing is written, gs_round reports it
    if (tid == 0) lvl[d] = start;
    const uint32_t nstart = start + qn;
    uint32_t nbase = 0;  // winners of the level's earlier trips
    for (uint32_t i0 = 0; i0 < qn; i0 += TWG_THREADS) {
      const uint32_t i = i0 + tid;
      const bool valid = i < qn;
      uint32_t u = 0, cand = 0;
      uint32_t dst[FP];
#pragma unroll
      for (int j = 0; j < FP; ++j) dst[j] = 0;
      // ---- claim
      if (valid) {
        u = q[start + i];
        const uint32_t nl = nl_l[u], head = nl & 31u;
        uint32_t row[ASZP];
        load_row<ASZP>(a.peers + (size_t)(u * NB + (nl >> 11)) * ASZP, row);
        const uint32_t pm = taken_slots<ASZP>(row, head, (nl >> 5) & 63u, a.ASZ, mk_l[u], org, fan);
        const uint32_t k = take_order<ASZP, FP>(row, pm, head, dst);
        uint32_t live = k >= 32 ? 0xFFFFFFFFu : (1u << k) - 1u;
        if (nf) {  // failed peers burn their take slot and are not pushed to (gossip.rs:538-541)
#pragma unroll
          for (int j = 0; j < FP; ++j)
            if ((uint32_t)j < k && a.frank[dst[j]] < nf) live &= ~(1u << j);
        }
#pragma unroll
        for (int j = 0; j < FP; ++j) {
          if (!((live >> j) & 1u)) continue;
          const uint32_t w = dst[j];
          if (hop[w] != 0xFF) continue;  // reached before this level, or won by an earlier trip of it
          cand |= 1u << j;
          atomicMin(&key[w], (i << 6) | (uint32_t)j);
        }
      }
      __syncthreads();
      // ---- win and count
      uint32_t win = 0;
#pragma unroll
      for (int j = 0; j < FP; ++j) {
        if (!((cand >> j) & 1u)) continue;
        const uint32_t w = dst[j];
        if (key[w] != ((i << 6) | (uint32_t)j)) continue;
        win |= 1u << j;
        hop[w] = (uint8_t)(d + 1);
        par[w] = (uint16_t)u;
      }
      if (valid) kids[u] = (uint8_t)__popc(win);
      uint32_t lower = 0, wt = 0;  // winners of the wave's lower lanes / of the whole wave
#pragma unroll
      for (int j = 0; j < FP; ++j) {
        const uint64_t bj = __ballot((win >> j) & 1u);
        lower += __builtin_amdgcn_mbcnt_hi((uint32_t)(bj >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bj, 0u));
        wt += (uint32_t)__popcll(bj);
      }
      if (lane == 0) wtot[wid] = wt;
      __syncthreads();
      // ---- place
      uint32_t pre = 0, tot = 0;
#pragma unroll
      for (uint32_t v = 0; v < TWG_WAVES; ++v) {
        const uint32_t x = wtot[v];
        tot += x;
        pre += v < wid ? x : 0u;
      }
      uint32_t idx = nstart + nbase + pre + lower;
#pragma unroll
      for (int j = 0; j < FP; ++j)
        if ((win >> j) & 1u) q[idx++] = (uint16_t)dst[j];
      nbase += tot;
      // (the next trip's claim touches key and reads hop, both settled by the barrier above; its
      // wave totals are written behind its own first barrier)
    }
    __syncthreads();
    start = nstart;
    qn = nbase;
  }

  // ---------------- subtree sizes: the queue backwards, one level at a time ------------------
  for (uint32_t v = tid; v < N; v += TWG_THREADS) sub[v] = 0;
  if (tid == 0) lvl[d] = start;  // (levels 0 .. d - 1 hold nodes; d <= 254)
  __syncthreads();
  for (uint32_t dd = d - 1; dd >= 1; --dd) {
    const uint32_t s0 = lvl[dd], s1 = lvl[dd + 1];
    for (uint32_t i = s0 + tid; i < s1; i += TWG_THREADS) {
      const uint32_t w = q[i];
      atomicAdd(&sub[par[w]], sub[w] + 1u);  // (sub[w] is final: w's children were the level before)
    }
    __syncthreads();
  }

  // ---------------- outputs: the workgroup owns its slot's pairs ----------------------------
  for (uint32_t v = tid; v < N; v += TWG_THREADS) {
    const size_t p = base + v;
    const uint32_t h = hop[v];
    nts(&out.parent[p], h != 0xFF && h != 0 ? (uint32_t)par[v] : 0xFFFFFFFFu);
    const uint32_t kd = kids[v], sb = sub[v];
    if (kd) out.kids_acc[p] += kd;
    if (sb) out.sub_acc[p] += sb;
  }
}

// One thread per node: the accumulators summed over every slot (coalesced across nodes).
__global__ __launch_bounds__(256) void k_tree_sum(const uint32_t* __restrict__ kids, const uint32_t* __restrict__ sub,
                                                  uint32_t N, uint32_t S, unsigned long long* __restrict__ okids,
                                                  unsigned long long* __restrict__ osub) {
  const uint32_t v = blockIdx.x * 256 + threadIdx.x;
  if (v >= N) return;
  unsigned long long ck = 0, cs = 0;
  for (uint32_t s = 0; s < S; ++s) {
    ck += kids[(size_t)s * N + v];
    cs += sub[(size_t)s * N + v];
  }
  okids[v] = ck;
  osub[v] = cs;
}

template <int ASZP, int FP>
static hipError_t launch_twg_fp(Engine& e, const RoundArgs& a, const TreeOut& out, size_t lds) {
  if (e.tr_attr_lds != lds || e.tr_attr_fp != FP) {  // (the attribute belongs to the instantiation; ASZP is the engine's)
    hipError_t r = hipFuncSetAttribute((const void*)k_tree_wg<ASZP, FP>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)lds);
    if (r != hipSuccess) return r;
    e.tr_attr_lds = lds;
    e.tr_attr_fp = FP;
  }
  hipLaunchKernelGGL((k_tree_wg<ASZP, FP>), dim3(e.S), dim3(TWG_THREADS), lds, e.st, a, out);
  return hipSuccess;
}

template <int ASZP>
static hipError_t launch_twg(Engine& e, const RoundArgs& a, const TreeOut& out, size_t lds) {
  // FP: push columns per lane (fanout <= 6, the reference's default, or the ring), as the round kernel's
  constexpr int FP6 = ASZP < 6 ? ASZP : 6;
  if (a.fcap <= (uint32_t)FP6) return launch_twg_fp<ASZP, FP6>(e, a, out, lds);
  return launch_twg_fp<ASZP, ASZP>(e, a, out, lds);
}

hipError_t launch_tree_wg(Engine& e, bool rot_clear) {
  // the arguments of the round's own launch (no rotation workgroup, no slot group): the current row
  // buffer, the masks before the round's prunes, the pending clear of the last rotation
  const RoundArgs a = round_args(e, true, e.sum_used, rot_clear, nullptr, nullptr);
  const TreeOut out{e.tr_parent, e.tr_kids, e.tr_sub};
  const size_t lds = tree_wg_lds_bytes(e.N, e.ASZP);
  if (e.N > tree_wg_max_nodes(e.ASZP) || lds > TREE_LDS_MAX) return hipErrorInvalidValue;  // (refused at enable)
  hipError_t r;
  GS_ASZP_DISPATCH(e.ASZP, r = launch_twg<A>(e, a, out, lds));
  if (r != hipSuccess) return r;
  return hipGetLastError();
}

hipError_t launch_tree_sum(Engine& e, unsigned long long* kids, unsigned long long* sub) {
  hipLaunchKernelGGL(k_tree_sum, dim3((e.N + 255) / 256), dim3(256), 0, e.st, e.tr_kids, e.tr_sub, e.N, e.S, kids, sub);
  return hipGetLastError();
}

}  // namespace gs
