// gs_tree_rec.hip -- the delivery tree of every slot from the step-wise round's inbound records.
//
// Cluster::mst (gossip.rs:580-591): parent[w] = the node that discovered w first in run_gossip's
// FIFO queue order. k_tree_wg (gs_tree_wg.hip) redoes a slot's BFS in one workgroup's LDS; this
// pass serves the engines whose gs_round launches the step kernels (any node count): after their
// BFS the hops, in-degrees and inbound records (hop << 24 | src) of every pair are in HBM, and the
// rows and prune masks are still the ones the BFS saw. The queue is BFS-ordered, so level d is
// q[start[d], start[d + 1]) with the starts from a histogram of the hops, and within level d + 1
// the order is (queue position of the first discoverer, take index in its push list):
//   - claim: a lane per node w of level d + 1 picks, among w's records of hop d + 1, the source
//     with the smallest queue position (u), finds w's take index t in u's taken ring slots and
//     sets bit t of cmask[u];
//   - scan: a lane per queue position of level d counts its node's child bits; a block-exclusive
//     scan and one total per block, then one small block per slot turns the totals into prefixes
//     (two passes: nothing waits on another workgroup);
//   - place: qpos[w] = start[d + 1] + block prefix + exclusive count at qpos[u] + child bits of u
//     below t; q[qpos[w]] = w.
// No sort, no grid barrier, no spin-wait: levels are separated by kernel launches. Subtree sizes
// come from walking the levels backwards, one launch per level. All per-pair arrays are slot-major
// (pair = slot * N + node), so a wave's consecutive nodes or queue positions are coalesced.
#include <algorithm>

#include "gs_device.h"
#include "gs_internal.h"

namespace gs {

constexpr uint32_t TRR_B = 256;     // block width of every kernel here; the scan's block width
constexpr uint32_t TRR_W = TRR_B / 64;
constexpr uint32_t TRR_IT = 4;      // nodes per thread of the per-pair passes
constexpr uint32_t TRR_LV = 520;    // per slot: 257 level starts, then 256 bucket cursors (padded)
constexpr uint32_t TRR_META = 257;  // deepest level, widest slot of each level; then hist [S][256]
constexpr uint32_t TRR_NONE = 0xFFFFFFFFu;

struct TrrArgs {
  const uint8_t* hops;
  const uint32_t* cnt;
  const uint32_t* inb;
  const uint32_t* mask;
  const uint8_t* bucket;
  const uint32_t* peers;
  const uint16_t* hl;
  const uint32_t* origin;
  const uint8_t* obkt;
  const uint32_t* sfan;  // null: every slot takes `fanout`
  const uint32_t* stab;  // null: one table
  const TrajDev* ttab;
  size_t t_rows, t_ents, mso, msu, PAIRS;
  uint32_t N, S, ASZ, fanout, capin, nbmax;
  uint32_t *q, *qpos, *lst, *cmask, *pt, *ex;  // [PAIRS] each; ex doubles as the round's subtree sizes
  uint32_t* btot;                              // [S][nbmax] scan block totals, then their prefixes
  uint32_t* lv;                                // [S][TRR_LV]
  uint32_t* meta;                              // [TRR_META + S * 256]
  uint32_t *parent, *kids_acc, *sub_acc;
  uint32_t* err;
};

// Exclusive prefix of x over the block's 256 threads (every thread calls it); *total = the sum.
__device__ inline uint32_t block_excl_scan(uint32_t x, uint32_t* wt, uint32_t* total) {
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
  const uint32_t incl = wave_incl_scan(x);
  if (lane == 63) wt[wid] = incl;
  __syncthreads();
  uint32_t pre = 0, tot = 0;
#pragma unroll
  for (uint32_t v = 0; v < TRR_W; ++v) {
    const uint32_t y = wt[v];
    tot += y;
    pre += v < wid ? y : 0u;
  }
  __syncthreads();  // (wt may be written again)
  *total = tot;
  return pre + incl - x;
}

// Per-slot histogram of the hops (LDS first, one global add per block and level); clears cmask.
__global__ __launch_bounds__(TRR_B) void k_trr_hist(TrrArgs a) {
  __shared__ uint32_t h[256];
  const uint32_t tid = threadIdx.x, o = blockIdx.y;
  const size_t base = (size_t)o * a.N;
  h[tid] = 0;
  __syncthreads();
#pragma unroll
  for (uint32_t k = 0; k < TRR_IT; ++k) {
    const uint32_t v = blockIdx.x * (TRR_B * TRR_IT) + k * TRR_B + tid;
    if (v >= a.N) break;
    atomicAdd(&h[a.hops[base + v]], 1u);
    a.cmask[base + v] = 0;
  }
  __syncthreads();
  if (tid != 255 && h[tid]) atomicAdd(&a.meta[TRR_META + o * 256 + tid], h[tid]);
}

// One block per slot: level starts and bucket cursors from the histogram, the deepest level and
// each level's widest slot for the host. A slot past the 253-hop limit gets empty levels.
__global__ __launch_bounds__(TRR_B) void k_trr_starts(TrrArgs a) {
  __shared__ uint32_t wt[TRR_W];
  const uint32_t tid = threadIdx.x, o = blockIdx.x;
  uint32_t c = tid != 255 ? a.meta[TRR_META + o * 256 + tid] : 0u;
  if (__syncthreads_or(tid >= 254 && c)) c = 0;  // (a node at hop 254: the BFS reports GS_ERANGE)
  uint32_t tot;
  const uint32_t ex = block_excl_scan(c, wt, &tot);
  uint32_t* lv = a.lv + (size_t)o * TRR_LV;
  lv[tid] = ex;
  lv[257 + tid] = ex;
  if (tid == 255) lv[256] = tot;
  if (c) {
    atomicMax(&a.meta[0], tid);
    atomicMax(&a.meta[1 + tid], c);
  }
}

// Nodes bucketed by hop into lst (any order inside a level): LDS ranks, one global cursor add
// per block and level. The origin opens the queue; the origin and unreached nodes get no parent.
__global__ __launch_bounds__(TRR_B) void k_trr_bucket(TrrArgs a) {
  __shared__ uint32_t lc[256], lb[256];
  const uint32_t tid = threadIdx.x, o = blockIdx.y;
  const size_t base = (size_t)o * a.N;
  uint32_t* lv = a.lv + (size_t)o * TRR_LV;
  if (lv[256] == 0) return;  // (past the hop limit: no tree this round)
  lc[tid] = 0;
  __syncthreads();
  uint32_t hp[TRR_IT], rk[TRR_IT];
#pragma unroll
  for (uint32_t k = 0; k < TRR_IT; ++k) {
    const uint32_t v = blockIdx.x * (TRR_B * TRR_IT) + k * TRR_B + tid;
    hp[k] = v < a.N ? (uint32_t)a.hops[base + v] : 0xFFu;
    rk[k] = hp[k] != 0xFFu ? atomicAdd(&lc[hp[k]], 1u) : 0u;
  }
  __syncthreads();
  if (tid != 255 && lc[tid]) lb[tid] = atomicAdd(&lv[257 + tid], lc[tid]);
  __syncthreads();
#pragma unroll
  for (uint32_t k = 0; k < TRR_IT; ++k) {
    const uint32_t v = blockIdx.x * (TRR_B * TRR_IT) + k * TRR_B + tid;
    if (v >= a.N) break;
    if (hp[k] == 0xFFu || hp[k] == 0) a.parent[base + v] = TRR_NONE;
    if (hp[k] == 0xFFu) continue;
    const uint32_t pos = lb[hp[k]] + rk[k];
    if (pos >= a.N) { atomicOr(a.err, ERR_BOUNDS); continue; }
    a.lst[base + pos] = v;
    if (hp[k] == 0) { a.q[base] = v; a.qpos[base + v] = 0; }
  }
}

// Take index of ring slot s among the taken slots `tk` (physical ring slots), counted from the
// ring's head: the rank take_order (gs_tree_wg.hip) gives the same slot.
__device__ inline uint32_t take_index(uint32_t tk, uint32_t head, uint32_t s) {
  const uint32_t below_head = (1u << head) - 1u;
  const uint32_t lower = tk & ((1u << s) - 1u);
  return s >= head ? (uint32_t)__popc(lower & ~below_head) : (uint32_t)__popc(tk & ~below_head) + (uint32_t)__popc(lower);
}

// Claim of level d1: one lane per node w of the level.
template <int ASZP>
__global__ __launch_bounds__(TRR_B) void k_trr_claim(TrrArgs a, uint32_t d1) {
  const uint32_t o = blockIdx.y;
  const uint32_t* lv = a.lv + (size_t)o * TRR_LV;
  const uint32_t s0 = lv[d1], s1 = lv[d1 + 1], i = s0 + blockIdx.x * TRR_B + threadIdx.x;
  if (i >= s1) return;
  const size_t base = (size_t)o * a.N;
  const uint32_t w = a.lst[base + i];
  const size_t p = base + w;
  const uint32_t c = min(a.cnt[p], a.capin);
  uint32_t u = TRR_NONE, uq = TRR_NONE;
  for (uint32_t j = 0; j < c; ++j) {  // the first discoverer: the pusher of the level before with the smallest position
    const uint32_t r = a.inb[(size_t)j * a.PAIRS + p];
    const uint32_t src = r & 0xFFFFFFu;
    if ((r >> 24) != d1 || src >= a.N) continue;
    const uint32_t qp = a.qpos[base + src];
    if (qp < uq) { uq = qp; u = src; }
  }
  a.pt[p] = TRR_NONE;
  if (u == TRR_NONE) { atomicOr(a.err, ERR_BOUNDS); return; }
  // u's entry for this origin in the slot's own table, its prune mask, the slot's fanout
  const uint32_t org = a.origin[o], ent = u * NB + min((uint32_t)a.bucket[u], (uint32_t)a.obkt[o]);
  const uint32_t* peers = a.peers;
  const uint16_t* hl = a.hl;
  uint32_t asz = a.ASZ;
  if (a.stab) {
    const uint32_t t = a.stab[o];
    peers += t * a.t_rows; hl += t * a.t_ents;
    asz = a.ttab[t].asz;
  }
  const uint32_t hv = hl[ent], head = hv & 0xFFu;
  uint32_t row[ASZP];
  load_row<ASZP>(peers + (size_t)ent * ASZP, row);
  const uint32_t tk = taken_slots<ASZP>(row, head, hv >> 8, asz, a.mask[o * a.mso + u * a.msu], org,
                                        a.sfan ? a.sfan[o] : a.fanout);
  uint32_t hit = 0;
#pragma unroll
  for (int s = 0; s < ASZP; ++s) hit |= (uint32_t)(row[s] == w) << s;
  hit &= tk;
  if (!hit) { atomicOr(a.err, ERR_BOUNDS); return; }  // (a recorded push that u's row does not take)
  const uint32_t t = take_index(tk, head, (uint32_t)__ffs((int)hit) - 1u);
  a.pt[p] = u | (t << 24);
  atomicOr(&a.cmask[base + u], 1u << t);
}

// Count and scan of level d: one lane per queue position.
__global__ __launch_bounds__(TRR_B) void k_trr_scan(TrrArgs a, uint32_t d) {
  __shared__ uint32_t wt[TRR_W];
  const uint32_t o = blockIdx.y;
  const uint32_t* lv = a.lv + (size_t)o * TRR_LV;
  const uint32_t s0 = lv[d], s1 = lv[d + 1];
  if (blockIdx.x * TRR_B >= s1 - s0) return;  // (block-uniform)
  const size_t base = (size_t)o * a.N;
  const uint32_t i = s0 + blockIdx.x * TRR_B + threadIdx.x;
  const uint32_t k = i < s1 ? (uint32_t)__popc(a.cmask[base + a.q[base + i]]) : 0u;
  uint32_t tot;
  const uint32_t ex = block_excl_scan(k, wt, &tot);
  if (i < s1) a.ex[base + i] = ex;
  if (threadIdx.x == 0) a.btot[(size_t)o * a.nbmax + blockIdx.x] = tot;
}

// One block per slot: level d's block totals become their exclusive prefixes, in place. Thread
// i owns the run [i * r, (i + 1) * r) of the totals.
__global__ __launch_bounds__(TRR_B) void k_trr_tops(TrrArgs a, uint32_t d) {
  __shared__ uint32_t wt[TRR_W];
  const uint32_t o = blockIdx.x, tid = threadIdx.x;
  const uint32_t* lv = a.lv + (size_t)o * TRR_LV;
  const uint32_t nb = (lv[d + 1] - lv[d] + TRR_B - 1) / TRR_B, r = (nb + TRR_B - 1) / TRR_B;
  uint32_t* bt = a.btot + (size_t)o * a.nbmax;
  const uint32_t j0 = min(tid * r, nb), j1 = min(j0 + r, nb);
  uint32_t s = 0;
  for (uint32_t j = j0; j < j1; ++j) s += bt[j];
  uint32_t tot;
  uint32_t run = block_excl_scan(s, wt, &tot);
  for (uint32_t j = j0; j < j1; ++j) {
    const uint32_t x = bt[j];
    bt[j] = run;
    run += x;
  }
}

// Place of level d1: one lane per node w of the level.
__global__ __launch_bounds__(TRR_B) void k_trr_place(TrrArgs a, uint32_t d1) {
  const uint32_t o = blockIdx.y;
  const uint32_t* lv = a.lv + (size_t)o * TRR_LV;
  const uint32_t sp = lv[d1 - 1], s0 = lv[d1], s1 = lv[d1 + 1], i = s0 + blockIdx.x * TRR_B + threadIdx.x;
  if (i >= s1) return;
  const size_t base = (size_t)o * a.N;
  const uint32_t w = a.lst[base + i];
  const size_t p = base + w;
  const uint32_t x = a.pt[p];
  if (x == TRR_NONE) return;  // (the claim raised the error)
  const uint32_t u = x & 0xFFFFFFu, t = x >> 24;
  const uint32_t uq = a.qpos[base + u];
  if (uq < sp || uq >= s0) { atomicOr(a.err, ERR_BOUNDS); return; }
  const uint32_t pos = s0 + a.btot[(size_t)o * a.nbmax + (uq - sp) / TRR_B] + a.ex[base + uq] +
                       (uint32_t)__popc(a.cmask[base + u] & ((1u << t) - 1u));
  if (pos >= s1) { atomicOr(a.err, ERR_BOUNDS); return; }
  a.qpos[p] = pos;
  a.q[base + pos] = w;
  a.parent[p] = u;
}

// After the last level: the round's child counts into the accumulator; the scan scratch becomes
// the round's subtree sizes (zero).
__global__ __launch_bounds__(TRR_B) void k_trr_kids(TrrArgs a) {
  const size_t base = (size_t)blockIdx.y * a.N;
#pragma unroll
  for (uint32_t k = 0; k < TRR_IT; ++k) {
    const uint32_t v = blockIdx.x * (TRR_B * TRR_IT) + k * TRR_B + threadIdx.x;
    if (v >= a.N) break;
    const uint32_t kd = (uint32_t)__popc(a.cmask[base + v]);
    if (kd) a.kids_acc[base + v] += kd;
    a.ex[base + v] = 0;
  }
}

// Level dd's nodes add their subtrees to their parents' (their own are final: their children
// were the launch before).
__global__ __launch_bounds__(TRR_B) void k_trr_up(TrrArgs a, uint32_t dd) {
  const uint32_t o = blockIdx.y;
  const uint32_t* lv = a.lv + (size_t)o * TRR_LV;
  const uint32_t i = lv[dd] + blockIdx.x * TRR_B + threadIdx.x;
  if (i >= lv[dd + 1]) return;
  const size_t base = (size_t)o * a.N;
  const uint32_t w = a.lst[base + i], x = a.pt[base + w];
  if (x == TRR_NONE) return;
  atomicAdd(&a.ex[base + (x & 0xFFFFFFu)], a.ex[base + w] + 1u);
}

__global__ __launch_bounds__(TRR_B) void k_trr_subacc(TrrArgs a) {
  const size_t base = (size_t)blockIdx.y * a.N;
#pragma unroll
  for (uint32_t k = 0; k < TRR_IT; ++k) {
    const uint32_t v = blockIdx.x * (TRR_B * TRR_IT) + k * TRR_B + threadIdx.x;
    if (v >= a.N) break;
    const uint32_t sb = a.ex[base + v];
    if (sb) a.sub_acc[base + v] += sb;
  }
}

size_t tree_rec_meta_words(const Engine& e) { return TRR_META + (size_t)e.S * 256; }
size_t tree_rec_lv_words(const Engine& e) { return (size_t)e.S * TRR_LV; }
size_t tree_rec_btot_words(const Engine& e) { return (size_t)e.S * ((e.N + TRR_B - 1) / TRR_B); }

template <int ASZP>
static void launch_claim(const TrrArgs& a, dim3 grid, hipStream_t st, uint32_t d1) {
  hipLaunchKernelGGL((k_trr_claim<ASZP>), grid, dim3(TRR_B), 0, st, a, d1);
}

// The whole pass of one recorded round, on e.st behind the round's BFS. The host reads the
// deepest level and each level's widest slot back once (1 KB) to bound the level loop and size
// its grids; *launches = kernels launched.
hipError_t launch_tree_rec(Engine& e, uint32_t* launches) {
  TrrArgs a;
  a.hops = e.hops; a.cnt = e.cnt; a.inb = e.inb; a.mask = e.mask; a.bucket = e.bucket; a.peers = e.peers; a.hl = e.hl;
  a.origin = e.origin; a.obkt = e.obkt; a.sfan = e.sfan;
  a.stab = e.T > 1 ? e.stab : nullptr; a.ttab = e.ttab; a.t_rows = e.t_rows; a.t_ents = e.t_ents;
  a.mso = e.mso; a.msu = e.msu; a.PAIRS = e.PAIRS;
  a.N = e.N; a.S = e.S; a.ASZ = e.ASZ; a.fanout = e.fanout; a.capin = e.capin; a.nbmax = (e.N + TRR_B - 1) / TRR_B;
  a.q = e.trr_q; a.qpos = e.trr_qpos; a.lst = e.trr_lst; a.cmask = e.trr_cmask; a.pt = e.trr_pt; a.ex = e.trr_ex;
  a.btot = e.trr_btot; a.lv = e.trr_lv; a.meta = e.trr_meta;
  a.parent = e.tr_parent; a.kids_acc = e.tr_kids; a.sub_acc = e.tr_sub; a.err = e.err;
  if (!a.inb || !a.q || e.PAIRS != (size_t)e.S * e.N) return hipErrorInvalidValue;
  const dim3 blk(TRR_B), pairs((e.N + TRR_B * TRR_IT - 1) / (TRR_B * TRR_IT), e.S);
  uint32_t n = 0;
  hipError_t r = hipMemsetAsync(e.trr_meta, 0, tree_rec_meta_words(e) * 4, e.st);
  if (r != hipSuccess) return r;
  hipLaunchKernelGGL(k_trr_hist, pairs, blk, 0, e.st, a);
  hipLaunchKernelGGL(k_trr_starts, dim3(e.S), blk, 0, e.st, a);
  hipLaunchKernelGGL(k_trr_bucket, pairs, blk, 0, e.st, a);
  n += 3;
  if ((r = hipGetLastError()) != hipSuccess) return r;
  r = hipMemcpyAsync(e.trr_hmeta, e.trr_meta, TRR_META * 4, hipMemcpyDeviceToHost, e.st);
  if (r == hipSuccess) r = hipStreamSynchronize(e.st);
  if (r != hipSuccess) return r;
  const uint32_t maxd = std::min(e.trr_hmeta[0], 253u);
  const uint32_t* wmax = e.trr_hmeta + 1;
  auto grid = [&](uint32_t d) { return dim3((wmax[d] + TRR_B - 1) / TRR_B, e.S); };
  for (uint32_t d = 0; d < maxd; ++d) {
    if (!wmax[d] || !wmax[d + 1]) break;  // (levels are contiguous: not reached)
    GS_ASZP_DISPATCH(e.ASZP, launch_claim<A>(a, grid(d + 1), e.st, d + 1));
    hipLaunchKernelGGL(k_trr_scan, grid(d), blk, 0, e.st, a, d);
    hipLaunchKernelGGL(k_trr_tops, dim3(e.S), blk, 0, e.st, a, d);
    hipLaunchKernelGGL(k_trr_place, grid(d + 1), blk, 0, e.st, a, d + 1);
    n += 4;
  }
  hipLaunchKernelGGL(k_trr_kids, pairs, blk, 0, e.st, a);
  for (uint32_t dd = maxd; dd >= 1; --dd) {
    if (!wmax[dd]) continue;
    hipLaunchKernelGGL(k_trr_up, grid(dd), blk, 0, e.st, a, dd);
    ++n;
  }
  hipLaunchKernelGGL(k_trr_subacc, pairs, blk, 0, e.st, a);
  n += 2;
  if (launches) *launches = n;
  return hipGetLastError();
}

}  // namespace gs
