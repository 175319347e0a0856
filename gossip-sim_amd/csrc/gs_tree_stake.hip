// gs_tree_stake.hip -- the delivery tree in stake: the stake below every node of every slot's
// tree, and its weighted sums per slot group (include/gossip_hip.h gs_tree_stake_*).
//
// After a recorded round with a tree mode on, three launches on the engine's stream read what the
// round left in HBM -- the parents gs_read_tree returns, the hop bytes gs_read_hops returns and the
// per-node stakes:
//
//   k_tstake_up      one workgroup per slot. The slot's nodes are counting-sorted by hop byte in
//                    LDS (a 256-bin histogram, a scan, a scatter into a level-ordered list whose
//                    entries carry node | parent << 16), then the levels are walked deepest first
//                    with one barrier per level: every node w of the level adds, with LDS atomics,
//                    what it holds to its parent p,
//                        at[p] += at[w]                       (u64: stake at or below the node)
//                        ks[p] += 1 << 16 | (sub[w] + 1)      (u32: kids << 16 | sub)
//                    at[] starts as the stakes (a coalesced load), so `below` is at[v] - stake[v]
//                    at the end (a second coalesced load) and the walk itself reads no global
//                    memory. A level wider than the workgroup takes several trips; a level's cost
//                    is its own width, so the 253-hop chain costs 253 barriers and not 253 scans
//                    of N. kids and sub share a word: both stay below N < 2^16, and one atomic
//                    serves both. The round's below (u64) and kids << 16 | sub (u32) are written
//                    coalesced to per-pair arrays, overwriting the previous round's.
//   k_tstake_reduce  grid (node blocks, chunks of gs_cluster_plan.h: a chunk lies in one group).
//                    A lane owns four consecutive nodes, a wave 256, and the block's four waves
//                    split the chunk's slots, so a slot's weight is uniform over the wave (a zero
//                    weight skips the slot's loads). Per node w kids, w sub, w lo32(below) and
//                    w hi32(below) are summed in u64 registers over the wave's slots; the waves
//                    meet in 8 KB of LDS and the block adds every non-zero word to the group's
//                    scratch [G][N][4] with one no-return u64 atomicAdd.
//   k_tstake_fold    one thread per (group, node), no atomics: scratch -> the round's 128-bit
//                    lo_sum + (hi_sum << 32) and its two counts, stored as the last round's values
//                    and added to the totals with carry; scratch zeroed for the next round.
//
// LDS of k_tstake_up: 16 B per node (at 8, ks 4, list 4) + 1,040 B, dynamic; ts_layout is shared
// by the host's size query and the kernel. Limbs: a group's round sums are at most (sum of weights)
// x n_nodes x (2^32 - 1), below 2^64 under gs_tree_stake_enable_groups' bound.
//
// Out-of-range input (after a round that raised the 253-hop error the parents and hops of a slot
// may belong to different rounds) changes values only: a parent >= N is no parent, the level loop
// ends at 253, and every LDS index is a node id below N or a list position below N.
#include "gs_device.h"
#include "gs_internal.h"

namespace gs {

namespace {

typedef unsigned long long u64;

constexpr uint32_t TS_THREADS = 512;  // k_tstake_up's workgroup
constexpr uint32_t TS_NODES = 256;    // nodes per block of the reduction (64 lanes x 4)
constexpr uint32_t TS_WORDS = 4;      // w kids, w sub, w lo32(below), w hi32(below)
constexpr uint32_t TS_NOPAR = 0xFFFFu;

static_assert(TS_NODES == CLUSTER_PLAN_NODES, "the chunk table is planned for the cluster view's node blocks");
static_assert(sizeof(ClusterChunk) == sizeof(uint3), "k_tstake_reduce reads a chunk as a uint3");

// LDS carve-up of k_tstake_up (byte offsets)
struct TsLayout {
  uint32_t bins, ctl, at, ks, list, total;
};
__host__ __device__ inline TsLayout ts_layout(uint32_t N) {
  TsLayout L;
  uint32_t o = 0;
  L.bins = o; o += 256 * 4;  // nodes per hop byte; after the scan a cursor; after the scatter each level's end
  L.ctl = o;  o += 16;       // [0] the deepest level that holds a node, [1..3] the scan's wave totals
  L.at = o;   o += 8 * N;    // stake at or below the node
  L.ks = o;   o += 4 * N;    // kids << 16 | sub
  L.list = o; o += 4 * N;    // nodes in level order: node | parent << 16 (TS_NOPAR: none)
  L.total = o;
  return L;
}

__global__ __launch_bounds__(TS_THREADS) void k_tstake_up(const uint32_t* __restrict__ parent,
                                                          const uint8_t* __restrict__ hops,
                                                          const uint64_t* __restrict__ stake, uint32_t N,
                                                          u64* __restrict__ below, uint32_t* __restrict__ ks_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const TsLayout L = ts_layout(N);
  uint32_t* bins = reinterpret_cast<uint32_t*>(smem + L.bins);
  uint32_t* ctl = reinterpret_cast<uint32_t*>(smem + L.ctl);
  u64* at = reinterpret_cast<u64*>(smem + L.at);
  uint32_t* ks = reinterpret_cast<uint32_t*>(smem + L.ks);
  uint32_t* list = reinterpret_cast<uint32_t*>(smem + L.list);
  const uint32_t tid = threadIdx.x;
  const size_t row = (size_t)blockIdx.x * N;
  const uint32_t* par = parent + row;
  const uint8_t* hop = hops + row;

  if (tid < 256) bins[tid] = 0;
  if (tid < 4) ctl[tid] = 0;
  __syncthreads();
  for (uint32_t v = tid; v < N; v += TS_THREADS) {
    at[v] = stake[v];
    ks[v] = 0;
    atomicAdd(&bins[hop[v]], 1u);
  }
  __syncthreads();
  // exclusive scan of the 256 bins: four waves scan 64 each, the first three's totals meet in ctl[1..3]
  uint32_t c = 0, incl = 0;
  if (tid < 256) {
    c = bins[tid];
    incl = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t up = __shfl_up(incl, o, 64);
      if ((tid & 63u) >= (uint32_t)o) incl += up;
    }
    if ((tid & 63u) == 63u && tid < 192) ctl[1 + (tid >> 6)] = incl;
    if (c && tid >= 1 && tid <= 253) atomicMax(&ctl[0], tid);
  }
  __syncthreads();
  if (tid < 256) {
    uint32_t base = 0;
    for (uint32_t w = 0; w < (tid >> 6); ++w) base += ctl[1 + w];
    bins[tid] = base + incl - c;
  }
  __syncthreads();
  for (uint32_t v = tid; v < N; v += TS_THREADS) {
    const uint32_t p = par[v];
    const uint32_t pos = atomicAdd(&bins[hop[v]], 1u);
    if (pos < N) list[pos] = v | (p < N ? p : TS_NOPAR) << 16;
  }
  __syncthreads();
  // bins[h] is now the end of level h in the list, so level h starts at bins[h - 1]
  const uint32_t deepest = min(ctl[0], 253u);
  for (uint32_t lv = deepest; lv >= 1; --lv) {
    const uint32_t lo = bins[lv - 1], hi = min(bins[lv], N);
    for (uint32_t i = lo + tid; i < hi; i += TS_THREADS) {
      const uint32_t ent = list[i];
      const uint32_t w = ent & 0xFFFFu, p = ent >> 16;
      if (p != TS_NOPAR) {
        atomicAdd(&at[p], at[w]);
        atomicAdd(&ks[p], 0x10001u + (ks[w] & 0xFFFFu));
      }
    }
    __syncthreads();
  }
  for (uint32_t v = tid; v < N; v += TS_THREADS) {
    below[row + v] = at[v] - stake[v];
    ks_out[row + v] = ks[v];
  }
}

// four consecutive kids / sub words, 16-byte aligned per load
__device__ inline void load_ks4(const uint32_t* __restrict__ ks, uint32_t (&k4)[4]) {
  const uint4 kk = *reinterpret_cast<const uint4*>(ks);
  k4[0] = kk.x; k4[1] = kk.y; k4[2] = kk.z; k4[3] = kk.w;
}
__device__ inline void load_ks4(const u64* __restrict__ ks, u64 (&k4)[4]) {
  const ulonglong2 k01 = *reinterpret_cast<const ulonglong2*>(ks), k23 = *reinterpret_cast<const ulonglong2*>(ks + 2);
  k4[0] = k01.x; k4[1] = k01.y; k4[2] = k23.x; k4[3] = k23.y;
}

// grid (node blocks, chunks): blockIdx.y indexes the chunk table {group, s_lo, s_hi}. SH: ks is
// kids << SH | sub (16: k_tstake_up's; 24: the records mode's, gs_tree_stake_rec.hip; 32 in a u64
// word: the dominator kind's, gs_tree_dom.hip, where a node may have n - 1 children)
template <uint32_t SH, typename KS = uint32_t>
__global__ __launch_bounds__(256) void k_tstake_reduce(const u64* __restrict__ below, const KS* __restrict__ ks,
                                                       uint32_t N, const uint3* __restrict__ chunks,
                                                       const uint32_t* __restrict__ wts, u64* __restrict__ scr) {
  __shared__ u64 meet[TS_WORDS][4][64];  // [word][node of the lane][lane]: a lane's adds hit its own bank
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // (uniform: the weights load as scalars)
  const uint32_t v0 = blockIdx.x * TS_NODES + lane * 4;
  const uint32_t nv = v0 < N ? min(4u, N - v0) : 0u;  // this lane's nodes in range
  const uint3 ch = chunks[blockIdx.y];
  const uint32_t per = (ch.z - ch.y + 3) / 4;
  const uint32_t s_lo = min(ch.z, ch.y + wave * per);
  const uint32_t s_hi = min(ch.z, s_lo + per);
#pragma unroll
  for (uint32_t w = 0; w < TS_WORDS; ++w) meet[w][wave][lane] = 0;
  __syncthreads();
  u64 sk[4] = {0, 0, 0, 0}, ss[4] = {0, 0, 0, 0}, sl[4] = {0, 0, 0, 0}, sh[4] = {0, 0, 0, 0};
  if (nv) {
    for (uint32_t j = s_lo; j < s_hi; ++j) {
      const uint32_t w = wts[j];
      if (!w) continue;  // (uniform: the slot is not read at all)
      const size_t p = (size_t)j * N + v0;
      u64 b[4] = {0, 0, 0, 0};
      KS k4[4] = {0, 0, 0, 0};
      if (nv == 4 && (p & 3) == 0) {  // 16-byte aligned: three wide loads (four with u64 counts)
        const ulonglong2 b01 = *reinterpret_cast<const ulonglong2*>(below + p);
        const ulonglong2 b23 = *reinterpret_cast<const ulonglong2*>(below + p + 2);
        b[0] = b01.x; b[1] = b01.y; b[2] = b23.x; b[3] = b23.y;
        load_ks4(ks + p, k4);
      } else {
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k)
          if (k < nv) {
            b[k] = below[p + k];
            k4[k] = ks[p + k];
          }
      }
#pragma unroll
      for (uint32_t k = 0; k < 4; ++k) {
        sk[k] += (u64)w * (uint32_t)(k4[k] >> SH);
        ss[k] += (u64)w * (uint32_t)(k4[k] & (((KS)1 << SH) - 1u));
        sl[k] += (u64)w * (uint32_t)b[k];
        sh[k] += (u64)w * (uint32_t)(b[k] >> 32);
      }
    }
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
      if (sk[k]) atomicAdd(&meet[0][k][lane], sk[k]);
      if (ss[k]) atomicAdd(&meet[1][k][lane], ss[k]);
      if (sl[k]) atomicAdd(&meet[2][k][lane], sl[k]);
      if (sh[k]) atomicAdd(&meet[3][k][lane], sh[k]);
    }
  }
  __syncthreads();
  const uint32_t v = blockIdx.x * TS_NODES + threadIdx.x;  // thread t takes node t of the block: lane t / 4, its node t % 4
  if (v < N) {
    u64* g = scr + ((size_t)ch.x * N + v) * TS_WORDS;
#pragma unroll
    for (uint32_t w = 0; w < TS_WORDS; ++w) {
      const u64 x = meet[w][threadIdx.x & 3u][threadIdx.x >> 2];
      if (x) atomicAdd(&g[w], x);
    }
  }
}

// One thread per (group, node). acc: per group [8][N] u64 -- children, subtree, below lo, below hi
// over the recorded rounds, then the same four of the last recorded round.
__global__ __launch_bounds__(256) void k_tstake_fold(u64* __restrict__ scr, u64* __restrict__ acc, uint32_t N,
                                                     uint32_t G) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)G * N) return;
  const size_t g = i / N, v = i - g * N;
  ulonglong2* s = reinterpret_cast<ulonglong2*>(scr + i * TS_WORDS);
  const ulonglong2 ksum = s[0], lim = s[1];
  s[0] = make_ulonglong2(0, 0);
  s[1] = make_ulonglong2(0, 0);
  u64* a = acc + g * 8 * N + v;
  const u64 rl = lim.x + (lim.y << 32);
  const u64 rh = (lim.y >> 32) + (rl < lim.x ? 1u : 0u);
  a[4 * (size_t)N] = ksum.x;
  a[5 * (size_t)N] = ksum.y;
  a[6 * (size_t)N] = rl;
  a[7 * (size_t)N] = rh;
  a[0] += ksum.x;
  a[1 * (size_t)N] += ksum.y;
  const u64 tl = a[2 * (size_t)N] + rl;
  a[2 * (size_t)N] = tl;
  a[3 * (size_t)N] += rh + (tl < rl ? 1u : 0u);
}

}  // namespace

size_t tree_stake_lds_bytes(uint32_t N) { return ts_layout(N).total; }

// LDS bytes per node, from the layout
uint32_t tree_stake_node_bytes() { return (uint32_t)((tree_stake_lds_bytes(4096) - tree_stake_lds_bytes(0)) / 4096); }

// Largest N k_tstake_up serves: the layout fits one workgroup's LDS (node ids, child counts and
// subtree sizes then fit their 16 bits as well).
uint32_t tree_stake_max_nodes() {
  uint32_t lo = 0, hi = TS_NOPAR - 1;
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1) / 2;
    if (tree_stake_lds_bytes(mid) <= TREE_LDS_MAX) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// The recorded round's three launches (Engine::ts_on; the scratch is zero between rounds).
hipError_t launch_tstake_up(Engine& e) {
  const size_t lds = tree_stake_lds_bytes(e.N);
  if (e.N > tree_stake_max_nodes() || e.NP != e.N) return hipErrorInvalidValue;  // (refused at enable)
  if (e.ts_attr_lds != lds) {
    hipError_t r = hipFuncSetAttribute((const void*)k_tstake_up, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (r != hipSuccess) return r;
    e.ts_attr_lds = lds;
  }
  k_tstake_up<<<e.S, TS_THREADS, lds, e.st>>>(e.tr_parent, e.hops, e.stake, e.N, reinterpret_cast<u64*>(e.ts_below),
                                              e.ts_ks);
  return hipGetLastError();
}

hipError_t launch_tstake_reduce(Engine& e) {
  const dim3 grid((e.N + TS_NODES - 1) / TS_NODES, e.ts_nchunks);
  const u64* below = reinterpret_cast<const u64*>(e.ts_below);
  const uint3* chunks = reinterpret_cast<const uint3*>(e.ts_chunks);
  u64* scr = reinterpret_cast<u64*>(e.ts_scr);
  if (e.ts_dom)
    k_tstake_reduce<32, u64><<<grid, 256, 0, e.st>>>(below, reinterpret_cast<const u64*>(e.ts_ks), e.N, chunks, e.ts_wts, scr);
  else if (e.ts_rec) k_tstake_reduce<24><<<grid, 256, 0, e.st>>>(below, e.ts_ks, e.N, chunks, e.ts_wts, scr);
  else k_tstake_reduce<16><<<grid, 256, 0, e.st>>>(below, e.ts_ks, e.N, chunks, e.ts_wts, scr);
  return hipGetLastError();
}

hipError_t launch_tstake_fold(Engine& e) {
  const size_t cells = (size_t)e.ts_G * e.N;
  k_tstake_fold<<<(uint32_t)((cells + 255) / 256), 256, 0, e.st>>>(reinterpret_cast<u64*>(e.ts_scr),
                                                                   reinterpret_cast<u64*>(e.ts_acc), e.N, e.ts_G);
  return hipGetLastError();
}

}  // namespace gs
