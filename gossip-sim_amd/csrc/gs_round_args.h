// gs_round_args.h -- the one-kernel round's argument block and the LDS-independent helpers
// that the round kernel (gs_round_wg.hip) and the delivery-tree kernel (gs_tree_wg.hip) share.
#pragma once
#include "gs_device.h"
#include "gs_internal.h"

namespace gs {

#ifndef GS_NT_STORES
#define GS_NT_STORES 1
#endif

struct RoundArgs {
  const uint64_t* stake;
  const uint8_t* bucket;
  const uint32_t* peers;
  const uint16_t* hl;
  const uint32_t* frank;
  const uint32_t* srank;
  const uint32_t* by_srank;
  const uint32_t* prank;     // rank by (stake desc, id asc): the prune order's tie-broken stake key
  const uint32_t* by_prank;
  const uint64_t* pstake;    // stake by prune rank
  const uint4* rinfo;        // by prune rank: {node id, 0, stake lo, stake hi}
  const uint32_t* origin;
  const uint8_t* obkt;
  const uint32_t* nfail;
  const uint32_t* min_ingress;
  const double* thr;
  uint32_t* slot_prunes;
  uint8_t* hops;
  uint32_t* cnt;
  uint32_t* mask;
  uint32_t* cmeta;
  uint32_t* ckey;  // [CACHE_CAP][PAIRS] slot words (ck_make)
  uint8_t* egress;
  uint8_t* prune_round;
  uint32_t* egress_acc;
  uint32_t* ingress_acc;
  uint32_t* prune_acc;
  uint32_t* strand;
  uint64_t* hist_acc;
  gs_round_summary* sum;  // this round's row [S] of the summary ring (record only)
  // the last rotation's pending prune-bit clear (null when none): replaced ring slots
  // of rotated node u's entry k are rot_changed[u * 25 + k]
  const uint32_t* rot_list;
  const uint32_t* rot_count;
  const uint32_t* rot_changed;
  // rotation ahead (rot_on): workgroup 0 runs Cluster::chance_to_rotate of round rround on
  // the other row buffer (rpeers / rhl), after copying the previous ahead rotation's
  // entries (plist / pcount) into it from the current one
  uint32_t rot_on;
  const uint64_t* P;
  const uint32_t* IX;
  uint32_t* rpeers;
  uint16_t* rhl;
  uint32_t* rlist;
  uint32_t* rcount;
  uint32_t* rchanged;
  const uint32_t* plist;
  const uint32_t* pcount;
  uint64_t seed;
  double rp;
  uint32_t rround;
  uint32_t* err;
  unsigned long long* phase_clk;  // optional: per-phase clock sums (thread 0 of each workgroup)
  uint32_t wave_c_max;            // in-degree bound of the wave consume path (64; 24 for path coverage)
  uint32_t N, S, ASZ, fanout, fcap;
  size_t PAIRS;
  int record;
  const uint32_t* sfan;  // [S] per-slot fanouts while they differ (the PF kernels), else null: every slot takes `fanout`
  // several trajectory tables (the MT kernels; else null): slot o reads table stab[o] -- peers / hl /
  // rpeers / rhl hold the tables t_rows words / t_ents entries apart, the rotation lists N words,
  // the changed bits t_ents words and the counters 2 words apart -- with ttab[t]'s size and
  // probability; rot_on is then the number of tables (one leading rotation workgroup each).
  // ttab[t].seed is the table's Philox key (the MT kernels draw DECIDE and ROTATE on it) and frank
  // holds the tables' fail ranks t_frank words apart (0: one array, the tables' keys are equal)
  const uint32_t* stab;
  const TrajDev* ttab;
  size_t t_rows, t_ents, t_frank;
  // round split (last, so that every other argument keeps its place): the ahead rotation before
  // plist's, whose entries the rotation workgroup copies too -- with three row generations the
  // other buffer is two rotations behind the current one (null: one rotation, or none)
  const uint32_t* plist2;
  const uint32_t* pcount2;
};

// The round's arguments as launch_round_wg passes them (gs_round_wg.hip): the whole engine, or
// with `sl` one slot group of a split round.
RoundArgs round_args(Engine& e, bool record, uint32_t rec_slot, bool rot_clear, const RotAhead* ra,
                     const SplitLaunch* sl);

// Streaming per-pair state (read or written once per round, ~0.5 GB/round at C2)
// goes through non-temporal loads/stores so that it does not evict the shared
// active-set rows (3.6 MB at C2) from L2.
template <class T>
__device__ inline T ntl(const T* p) { return __builtin_nontemporal_load(p); }
template <class T>
__device__ inline void nts(T* p, T v) {
#if GS_NT_STORES
  __builtin_nontemporal_store(v, p);
#else
  *p = v;
#endif
}

}  // namespace gs
