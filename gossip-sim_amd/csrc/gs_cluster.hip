// gs_cluster.hip -- the cluster load view: per-node message load summed over every slot
// (include/gossip_hip.h gs_cluster_*).
//
// The reference's egress / ingress / prune trackers (gossip_stats.rs:359-461) are per origin;
// when every node originates, what one node sends and receives is the sum over the slots.
// After a recorded round's last kernel, two launches on the engine's stream read the pair
// arrays the round left -- exactly what gs_read_counters / gs_read_hops return per slot:
//
//   k_cluster_reduce  sums over slots into u32 scratch [5][NP]: egress (0 where the slot did
//                     not reach the node: that byte is stale), ingress, prunes sent,
//                     deliveries (1 <= hops <= 254) and their hops. A lane owns four
//                     consecutive nodes (one u32 load of four hop / egress / prune bytes, one
//                     uint4 of in-degrees; byte and word loads where slot * NP is no multiple
//                     of 4 or the node group is cut by NP), a wave 256 nodes, and the slots
//                     are split over the block's four waves and over gridDim.y chunks. The
//                     waves' partial sums meet in LDS; one no-return atomicAdd per node and
//                     word per block, 64 consecutive words per wave-instruction, zeros skipped.
//   k_cluster_fold    one thread per node, no atomics on per-node state: scratch -> u64
//                     totals, peaks, scratch zeroed for the next round; the round's scalars and
//                     (max, smallest id) are block-reduced and met in the round's ring entry by
//                     one u64 atomic per block and field (integer sums and maxima: order-free).
//
// Egress is slot-major (workgroup, level, binned engines) or node-major [node][SP] (multi,
// hybrid; SP = slots rounded up to 4, the pad bytes are not slots): there a lane loads the
// u32 of four slots of each of its nodes and walks the slots in fours.
#include <algorithm>

#include "gs_device.h"
#include "gs_internal.h"

namespace gs {

namespace {

constexpr uint32_t CL_NODES = 256;  // nodes per block (64 lanes x 4)
constexpr uint32_t CL_WORDS = 5;    // egress, ingress, prunes, delivered, hop sum

struct ClAcc { uint32_t e[4], i[4], p[4], d[4], h[4]; };
static_assert(sizeof(gs_cluster_round) == 7 * sizeof(unsigned long long), "k_cluster_fold writes 7 u64 words");

// four nodes of one slot: hop / egress / prune bytes packed in u32s, in-degrees in c
__device__ __forceinline__ void cl_add(ClAcc& a, uint32_t h, uint32_t eg, uint32_t pr, const uint4& c) {
  const uint32_t cc[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t hb = (h >> (8 * k)) & 0xFFu;
    const bool del = hb >= 1u && hb != (uint32_t)GS_HOP_UNREACHED;
    a.e[k] += hb != (uint32_t)GS_HOP_UNREACHED ? (eg >> (8 * k)) & 0xFFu : 0u;
    a.i[k] += cc[k];
    a.p[k] += (pr >> (8 * k)) & 0xFFu;
    a.d[k] += del ? 1u : 0u;
    a.h[k] += del ? hb : 0u;
  }
}

// up to four consecutive bytes / words at p (nv of them in range), packed like the vector loads
__device__ __forceinline__ uint32_t cl_bytes(const uint8_t* a, size_t p, uint32_t nv, bool vec, uint32_t fill) {
  if (vec) return *reinterpret_cast<const uint32_t*>(a + p);
  uint32_t w = 0;
#pragma unroll
  for (uint32_t k = 0; k < 4; ++k) w |= (k < nv ? (uint32_t)a[p + k] : fill) << (8 * k);
  return w;
}
__device__ __forceinline__ uint4 cl_words(const uint32_t* a, size_t p, uint32_t nv, bool vec) {
  if (vec) return *reinterpret_cast<const uint4*>(a + p);
  uint4 c;
  c.x = nv > 0 ? a[p] : 0u;
  c.y = nv > 1 ? a[p + 1] : 0u;
  c.z = nv > 2 ? a[p + 2] : 0u;
  c.w = nv > 3 ? a[p + 3] : 0u;
  return c;
}

// grid (node blocks, slot chunks of CH slots; CH a multiple of 16: a wave takes CH / 4 slots)
template <bool NODE_MAJOR>
__global__ __launch_bounds__(256) void k_cluster_reduce(const uint8_t* __restrict__ hops,
                                                        const uint32_t* __restrict__ cnt,
                                                        const uint8_t* __restrict__ prune_round,
                                                        const uint8_t* __restrict__ egress, uint32_t NP, uint32_t S,
                                                        uint32_t SP, uint32_t CH, uint32_t* __restrict__ scr) {
  __shared__ __attribute__((aligned(16))) uint32_t red[4][CL_WORDS][CL_NODES];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t v0 = blockIdx.x * CL_NODES + lane * 4;
  const uint32_t nv = v0 < NP ? min(4u, NP - v0) : 0u;  // this lane's nodes in range
  const uint32_t s_lo = blockIdx.y * CH + wave * (CH / 4);
  const uint32_t s_hi = min(S, s_lo + CH / 4);
  ClAcc a = {};
  if (nv) {
    if (!NODE_MAJOR) {
#pragma unroll 2
      for (uint32_t j = s_lo; j < s_hi; ++j) {
        const size_t p = (size_t)j * NP + v0;
        const bool vec = nv == 4 && (p & 3) == 0;
        const uint32_t h = cl_bytes(hops, p, nv, vec, GS_HOP_UNREACHED);
        const uint32_t eg = cl_bytes(egress, p, nv, vec, 0);
        const uint32_t pr = cl_bytes(prune_round, p, nv, vec, 0);
        cl_add(a, h, eg, pr, cl_words(cnt, p, nv, vec));
      }
    } else {
      for (uint32_t q = s_lo; q < s_hi; q += 4) {  // (q is a multiple of 4 and q + 3 < SP)
        uint32_t ew[4];
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k)
          ew[k] = k < nv ? *reinterpret_cast<const uint32_t*>(egress + (size_t)(v0 + k) * SP + q) : 0u;
#pragma unroll
        for (uint32_t jj = 0; jj < 4; ++jj) {
          const uint32_t j = q + jj;
          if (j >= s_hi) break;  // (the pad bytes of the last word are not slots)
          const size_t p = (size_t)j * NP + v0;
          const bool vec = nv == 4 && (p & 3) == 0;
          const uint32_t eg = ((ew[0] >> (8 * jj)) & 0xFFu) | (((ew[1] >> (8 * jj)) & 0xFFu) << 8) |
                              (((ew[2] >> (8 * jj)) & 0xFFu) << 16) | (((ew[3] >> (8 * jj)) & 0xFFu) << 24);
          const uint32_t h = cl_bytes(hops, p, nv, vec, GS_HOP_UNREACHED);
          const uint32_t pr = cl_bytes(prune_round, p, nv, vec, 0);
          cl_add(a, h, eg, pr, cl_words(cnt, p, nv, vec));
        }
      }
    }
  }
  *reinterpret_cast<uint4*>(&red[wave][0][lane * 4]) = make_uint4(a.e[0], a.e[1], a.e[2], a.e[3]);
  *reinterpret_cast<uint4*>(&red[wave][1][lane * 4]) = make_uint4(a.i[0], a.i[1], a.i[2], a.i[3]);
  *reinterpret_cast<uint4*>(&red[wave][2][lane * 4]) = make_uint4(a.p[0], a.p[1], a.p[2], a.p[3]);
  *reinterpret_cast<uint4*>(&red[wave][3][lane * 4]) = make_uint4(a.d[0], a.d[1], a.d[2], a.d[3]);
  *reinterpret_cast<uint4*>(&red[wave][4][lane * 4]) = make_uint4(a.h[0], a.h[1], a.h[2], a.h[3]);
  __syncthreads();
  const uint32_t v = blockIdx.x * CL_NODES + threadIdx.x;
  if (v >= NP) return;
#pragma unroll
  for (uint32_t w = 0; w < CL_WORDS; ++w) {
    const uint32_t x = red[0][w][threadIdx.x] + red[1][w][threadIdx.x] + red[2][w][threadIdx.x] +
                       red[3][w][threadIdx.x];
    if (x) atomicAdd(&scr[(size_t)w * NP + v], x);
  }
}

__device__ __forceinline__ unsigned long long cl_wave_sum(unsigned long long x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
  return x;
}
__device__ __forceinline__ unsigned long long cl_wave_max(unsigned long long x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long y = __shfl_down(x, o, 64);
    x = y > x ? y : x;
  }
  return x;
}

// One thread per node. out: the round's ring entry as 7 u64 words (zero before the launch):
// pushes, ingress, prunes, delivered, two keys (max << 32 | ~node: the largest key is the
// largest load and, among equals, the smallest id), senders. gs_engine.hip's drain turns the
// keys into gs_cluster_round's (max, node) fields.
__global__ __launch_bounds__(256) void k_cluster_fold(uint32_t* __restrict__ scr, unsigned long long* __restrict__ tot,
                                                      uint32_t* __restrict__ peak, uint32_t NP,
                                                      unsigned long long* __restrict__ out) {
  __shared__ unsigned long long red[4][7];
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  unsigned long long r[7] = {0, 0, 0, 0, 0, 0, 0};
  if (v < NP) {
    uint32_t x[CL_WORDS];
#pragma unroll
    for (uint32_t w = 0; w < CL_WORDS; ++w) {
      x[w] = scr[(size_t)w * NP + v];
      scr[(size_t)w * NP + v] = 0;
      if (x[w]) tot[(size_t)w * NP + v] += x[w];
    }
    if (x[0] > peak[v]) peak[v] = x[0];
    if (x[1] > peak[(size_t)NP + v]) peak[(size_t)NP + v] = x[1];
    r[0] = x[0]; r[1] = x[1]; r[2] = x[2]; r[3] = x[3];
    r[4] = ((unsigned long long)x[0] << 32) | (uint32_t)~v;
    r[5] = ((unsigned long long)x[1] << 32) | (uint32_t)~v;
    r[6] = x[0] ? 1u : 0u;
  }
#pragma unroll
  for (int k = 0; k < 7; ++k) r[k] = (k == 4 || k == 5) ? cl_wave_max(r[k]) : cl_wave_sum(r[k]);
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  if (lane == 0)
    for (int k = 0; k < 7; ++k) red[wave][k] = r[k];
  __syncthreads();
  if (threadIdx.x < 7) {
    const uint32_t k = threadIdx.x;
    unsigned long long x = red[0][k];
    for (uint32_t w = 1; w < 4; ++w) x = (k == 4 || k == 5) ? (red[w][k] > x ? red[w][k] : x) : x + red[w][k];
    if (k == 4 || k == 5) atomicMax(&out[k], x);
    else if (x) atomicAdd(&out[k], x);
  }
}

// ---- the grouped, weighted view (gs_cluster_enable_groups) ----
// The slots are cut into G groups of consecutive slots and slot j counts w_j times (0: not at
// all). Scratch, totals and peaks are [G][..][NP], the ring [round][G]. Still two launches.

// cl_add with the slot's weight (uniform over the wave)
__device__ __forceinline__ void cl_add_w(ClAcc& a, uint32_t h, uint32_t eg, uint32_t pr, const uint4& c, uint32_t w) {
  const uint32_t cc[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t hb = (h >> (8 * k)) & 0xFFu;
    const bool del = hb >= 1u && hb != (uint32_t)GS_HOP_UNREACHED;
    a.e[k] += hb != (uint32_t)GS_HOP_UNREACHED ? w * ((eg >> (8 * k)) & 0xFFu) : 0u;
    a.i[k] += w * cc[k];
    a.p[k] += w * ((pr >> (8 * k)) & 0xFFu);
    a.d[k] += del ? w : 0u;
    a.h[k] += del ? w * hb : 0u;
  }
}

// grid (node blocks, chunks): blockIdx.y indexes the chunk table (gs_cluster_plan.h: a chunk lies
// in one group), the block's four waves split the chunk's slots, and the sums go to the group's
// scratch [5][NP]. A wave's slot range [s_lo, s_hi) may begin and end anywhere: on node-major
// egress it walks the 4-slot words from s_lo & ~3 (a word starts below S, so it ends within SP)
// and skips the bytes outside the range -- another wave's or group's slots, or the pad.
template <bool NODE_MAJOR>
__global__ __launch_bounds__(256) void k_cluster_reduce_g(const uint8_t* __restrict__ hops,
                                                          const uint32_t* __restrict__ cnt,
                                                          const uint8_t* __restrict__ prune_round,
                                                          const uint8_t* __restrict__ egress, uint32_t NP, uint32_t SP,
                                                          const uint3* __restrict__ chunks,
                                                          const uint32_t* __restrict__ wts, uint32_t* __restrict__ scr) {
  __shared__ __attribute__((aligned(16))) uint32_t red[4][CL_WORDS][CL_NODES];
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // (uniform: the weights load as scalars)
  const uint32_t v0 = blockIdx.x * CL_NODES + lane * 4;
  const uint32_t nv = v0 < NP ? min(4u, NP - v0) : 0u;  // this lane's nodes in range
  const uint3 ch = chunks[blockIdx.y];                  // {group, s_lo, s_hi}
  uint32_t per = (ch.z - ch.y + 3) / 4;
  if (NODE_MAJOR) per = (per + 3u) & ~3u;  // (whole words per wave where the chunk starts on one)
  const uint32_t s_lo = min(ch.z, ch.y + wave * per);
  const uint32_t s_hi = min(ch.z, s_lo + per);
  ClAcc a = {};
  if (nv) {
    if (!NODE_MAJOR) {
#pragma unroll 2
      for (uint32_t j = s_lo; j < s_hi; ++j) {
        const uint32_t w = wts[j];  // (0: the slot adds nothing; no branch, so two slots' loads overlap)
        const size_t p = (size_t)j * NP + v0;
        const bool vec = nv == 4 && (p & 3) == 0;
        const uint32_t h = cl_bytes(hops, p, nv, vec, GS_HOP_UNREACHED);
        const uint32_t eg = cl_bytes(egress, p, nv, vec, 0);
        const uint32_t pr = cl_bytes(prune_round, p, nv, vec, 0);
        cl_add_w(a, h, eg, pr, cl_words(cnt, p, nv, vec), w);
      }
    } else {
      for (uint32_t q = s_lo & ~3u; q < s_hi; q += 4) {  // (q is a multiple of 4 below S, so q + 3 < SP)
        uint32_t ew[4];
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k)
          ew[k] = k < nv ? *reinterpret_cast<const uint32_t*>(egress + (size_t)(v0 + k) * SP + q) : 0u;
#pragma unroll
        for (uint32_t jj = 0; jj < 4; ++jj) {
          const uint32_t j = q + jj;
          if (j < s_lo) continue;  // (slots before the range: not this wave's, maybe not this group's)
          if (j >= s_hi) break;    // (and behind it; the pad bytes of the last word are not slots)
          const uint32_t w = wts[j];
          const size_t p = (size_t)j * NP + v0;
          const bool vec = nv == 4 && (p & 3) == 0;
          const uint32_t eg = ((ew[0] >> (8 * jj)) & 0xFFu) | (((ew[1] >> (8 * jj)) & 0xFFu) << 8) |
                              (((ew[2] >> (8 * jj)) & 0xFFu) << 16) | (((ew[3] >> (8 * jj)) & 0xFFu) << 24);
          const uint32_t h = cl_bytes(hops, p, nv, vec, GS_HOP_UNREACHED);
          const uint32_t pr = cl_bytes(prune_round, p, nv, vec, 0);
          cl_add_w(a, h, eg, pr, cl_words(cnt, p, nv, vec), w);
        }
      }
    }
  }
  *reinterpret_cast<uint4*>(&red[wave][0][lane * 4]) = make_uint4(a.e[0], a.e[1], a.e[2], a.e[3]);
  *reinterpret_cast<uint4*>(&red[wave][1][lane * 4]) = make_uint4(a.i[0], a.i[1], a.i[2], a.i[3]);
  *reinterpret_cast<uint4*>(&red[wave][2][lane * 4]) = make_uint4(a.p[0], a.p[1], a.p[2], a.p[3]);
  *reinterpret_cast<uint4*>(&red[wave][3][lane * 4]) = make_uint4(a.d[0], a.d[1], a.d[2], a.d[3]);
  *reinterpret_cast<uint4*>(&red[wave][4][lane * 4]) = make_uint4(a.h[0], a.h[1], a.h[2], a.h[3]);
  __syncthreads();
  const uint32_t v = blockIdx.x * CL_NODES + threadIdx.x;
  if (v >= NP) return;
  uint32_t* gscr = scr + (size_t)ch.x * CL_WORDS * NP;
#pragma unroll
  for (uint32_t w = 0; w < CL_WORDS; ++w) {
    const uint32_t x = red[0][w][threadIdx.x] + red[1][w][threadIdx.x] + red[2][w][threadIdx.x] +
                       red[3][w][threadIdx.x];
    if (x) atomicAdd(&gscr[(size_t)w * NP + v], x);
  }
}

// k_cluster_fold per group: grid (node blocks, G). Group g's scratch goes to its totals and peaks
// and is zeroed; out is the round's G ring entries, group g's the 7 u64 words at 7 g.
__global__ __launch_bounds__(256) void k_cluster_fold_g(uint32_t* __restrict__ scr, unsigned long long* __restrict__ tot,
                                                        uint32_t* __restrict__ peak, uint32_t NP,
                                                        unsigned long long* __restrict__ out) {
  __shared__ unsigned long long red[4][7];
  const uint32_t g = blockIdx.y;
  scr += (size_t)g * CL_WORDS * NP;
  tot += (size_t)g * CL_WORDS * NP;
  peak += (size_t)g * 2 * NP;
  out += (size_t)g * 7;
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  unsigned long long r[7] = {0, 0, 0, 0, 0, 0, 0};
  if (v < NP) {
    uint32_t x[CL_WORDS];
#pragma unroll
    for (uint32_t w = 0; w < CL_WORDS; ++w) {
      x[w] = scr[(size_t)w * NP + v];
      scr[(size_t)w * NP + v] = 0;
      if (x[w]) tot[(size_t)w * NP + v] += x[w];
    }
    if (x[0] > peak[v]) peak[v] = x[0];
    if (x[1] > peak[(size_t)NP + v]) peak[(size_t)NP + v] = x[1];
    r[0] = x[0]; r[1] = x[1]; r[2] = x[2]; r[3] = x[3];
    r[4] = ((unsigned long long)x[0] << 32) | (uint32_t)~v;
    r[5] = ((unsigned long long)x[1] << 32) | (uint32_t)~v;
    r[6] = x[0] ? 1u : 0u;
  }
#pragma unroll
  for (int k = 0; k < 7; ++k) r[k] = (k == 4 || k == 5) ? cl_wave_max(r[k]) : cl_wave_sum(r[k]);
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  if (lane == 0)
    for (int k = 0; k < 7; ++k) red[wave][k] = r[k];
  __syncthreads();
  if (threadIdx.x < 7) {
    const uint32_t k = threadIdx.x;
    unsigned long long x = red[0][k];
    for (uint32_t w = 1; w < 4; ++w) x = (k == 4 || k == 5) ? (red[w][k] > x ? red[w][k] : x) : x + red[w][k];
    if (k == 4 || k == 5) atomicMax(&out[k], x);
    else if (x) atomicAdd(&out[k], x);
  }
}

static_assert(sizeof(ClusterChunk) == sizeof(uint3), "k_cluster_reduce_g reads a chunk as a uint3");

}  // namespace

// Slots per chunk of k_cluster_reduce's gridDim.y: enough blocks for ~8 per CU (C2: 12 node
// blocks x 94 chunks of 32 slots; C4: 3,907 node blocks x 1 chunk), a multiple of 16.
uint32_t cluster_chunk_slots(uint32_t NP, uint32_t S) {
  const uint32_t nb = (NP + CL_NODES - 1) / CL_NODES;
  const uint32_t want = std::max(1u, (2048u + nb - 1) / nb);
  const uint32_t per = (S + want - 1) / want;
  return std::max(16u, (per + 15u) & ~15u);
}

// ... of a grouped view (Engine::cl_grouped; the round's G ring entries are zero)
static hipError_t launch_cluster_view_g(Engine& e, uint32_t rec_index) {
  const uint32_t NP = e.NP, G = e.cl_G;
  const dim3 grid((NP + CL_NODES - 1) / CL_NODES, e.cl_nchunks);
  const uint3* chunks = reinterpret_cast<const uint3*>(e.cl_chunks);  // (ClusterChunk: three u32)
  if (e.esu == 1)
    k_cluster_reduce_g<false><<<grid, 256, 0, e.st>>>(e.hops, e.cnt, e.prune_round, e.egress, NP, e.SP, chunks, e.cl_wts,
                                                      e.cl_scr);
  else
    k_cluster_reduce_g<true><<<grid, 256, 0, e.st>>>(e.hops, e.cnt, e.prune_round, e.egress, NP, e.SP, chunks, e.cl_wts,
                                                     e.cl_scr);
  hipError_t r = hipGetLastError();
  if (r != hipSuccess) return r;
  k_cluster_fold_g<<<dim3((NP + 255) / 256, G), 256, 0, e.st>>>(
      e.cl_scr, reinterpret_cast<unsigned long long*>(e.cl_tot), e.cl_peak, NP,
      reinterpret_cast<unsigned long long*>(e.cl_ring + (size_t)rec_index * G));
  return hipGetLastError();
}

// The recorded round `rec_index`'s reduction (Engine::cl_on; the ring entry is zero).
hipError_t launch_cluster_view(Engine& e, uint32_t rec_index) {
  if (e.cl_grouped) return launch_cluster_view_g(e, rec_index);
  const uint32_t NP = e.NP, S = e.S;
  const uint32_t CH = cluster_chunk_slots(NP, S);
  const dim3 grid((NP + CL_NODES - 1) / CL_NODES, (S + CH - 1) / CH);
  if (e.esu == 1)
    k_cluster_reduce<false><<<grid, 256, 0, e.st>>>(e.hops, e.cnt, e.prune_round, e.egress, NP, S, e.SP, CH, e.cl_scr);
  else
    k_cluster_reduce<true><<<grid, 256, 0, e.st>>>(e.hops, e.cnt, e.prune_round, e.egress, NP, S, e.SP, CH, e.cl_scr);
  hipError_t r = hipGetLastError();
  if (r != hipSuccess) return r;
  k_cluster_fold<<<(NP + 255) / 256, 256, 0, e.st>>>(
      e.cl_scr, reinterpret_cast<unsigned long long*>(e.cl_tot), e.cl_peak, NP,
      reinterpret_cast<unsigned long long*>(e.cl_ring + rec_index));
  return hipGetLastError();
}

}  // namespace gs
