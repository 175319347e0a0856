// Stand-alone check of the multi-source BFS's host-side group-table builder (gs_mv_groups.h)
// for engines of several trajectory tables. Built and run by tests/test_traj_multi_cpu.py with
// the host compiler's address and undefined-behaviour sanitizers; prints "ok" and exits 0, or
// names the first property that fails.
//
// Layout (GW = 28, as at every node count up to 2^27): 32 slots, four tables of eight slots,
// so the groups are slots 0..27 and 28..31 and table 3 (slots 24..31) straddles the boundary.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>
#include <vector>

#include "gs_mv_groups.h"

using namespace gs;

#define CHECK(c)                                                \
  do {                                                          \
    if (!(c)) {                                                 \
      std::fprintf(stderr, "line %d: %s\n", __LINE__, #c);      \
      return 1;                                                 \
    }                                                           \
  } while (0)

static int check(uint32_t S, uint32_t GW, const std::vector<uint32_t>& origins, const std::vector<uint8_t>& bucket,
                 const std::vector<uint32_t>* stab) {
  std::vector<uint8_t> obkt(S);
  for (uint32_t o = 0; o < S; ++o) obkt[o] = bucket[origins[o]];
  // exact-size heap buffers: a read or write past any input or output trips the sanitizer
  std::vector<uint32_t> gtab;
  std::vector<MvSeed> seeds;
  std::vector<MvGroup> groups;
  mv_groups_build(S, GW, origins.data(), obkt.data(), bucket.data(), stab ? stab->data() : nullptr, gtab, seeds, groups);
  const uint32_t ng = (S + GW - 1) / GW;
  CHECK(groups.size() == ng);
  CHECK(gtab.size() == (size_t)ng * GT_STRIDE);
  CHECK(seeds.size() <= S);
  std::set<uint32_t> seen_tables;
  uint32_t seed_at = 0;
  for (uint32_t g = 0; g < ng; ++g) {
    const uint32_t* t = gtab.data() + (size_t)g * GT_STRIDE;
    const uint32_t s0 = g * GW, sg = std::min(GW, S - s0);
    const uint32_t all = sg == 32 ? 0xFFFFFFFFu : (1u << sg) - 1u;
    CHECK(groups[g].s0 == s0 && groups[g].sg == sg && t[GT_S0] == s0 && t[GT_SG] == sg);
    // the table masks partition the group's slots, and each names the slots of its table
    const uint32_t nt = t[GT_NT];
    CHECK(nt >= 1 && nt <= sg && nt <= MV_GW_MAX);
    uint32_t uni = 0;
    for (uint32_t i = 0; i < nt; ++i) {
      const uint32_t m = t[GT_TM + i];
      CHECK(m != 0 && (m & uni) == 0 && (m & ~all) == 0);
      uni |= m;
      for (uint32_t j = 0; j < sg; ++j)
        if ((m >> j) & 1u) CHECK((stab ? (*stab)[s0 + j] : 0u) == t[GT_TI + i]);
      for (uint32_t k = 0; k < i; ++k) CHECK(t[GT_TI + k] != t[GT_TI + i]);
      seen_tables.insert(t[GT_TI + i] | (g << 16));
    }
    CHECK(uni == all);
    for (uint32_t i = nt; i < MV_GW_MAX; ++i) CHECK(t[GT_TM + i] == 0);
    // the seeds: one per distinct (origin, table), masks partition the group's slots, each
    // mask inside one table, at the origin's own entry
    CHECK(groups[g].seed0 == seed_at && t[GT_SEED] == seed_at && t[GT_NSEED] == groups[g].nseed);
    std::set<std::pair<uint32_t, uint32_t>> want, got;
    for (uint32_t j = 0; j < sg; ++j) want.insert({origins[s0 + j], stab ? (*stab)[s0 + j] : 0u});
    uint32_t su = 0;
    for (uint32_t i = 0; i < groups[g].nseed; ++i) {
      const MvSeed sd = seeds[seed_at + i];
      const uint32_t org = sd.x & 0xFFFFFFu;
      CHECK((sd.x >> 24) == bucket[org]);
      CHECK(sd.y != 0 && (sd.y & su) == 0 && (sd.y & ~all) == 0);
      su |= sd.y;
      uint32_t tb = 0xFFFFFFFFu;
      for (uint32_t j = 0; j < sg; ++j)
        if ((sd.y >> j) & 1u) {
          CHECK(origins[s0 + j] == org);
          const uint32_t x = stab ? (*stab)[s0 + j] : 0u;
          CHECK(tb == 0xFFFFFFFFu || tb == x);
          tb = x;
        }
      CHECK(got.insert({org, tb}).second);
    }
    CHECK(su == all && got == want);
    seed_at += groups[g].nseed;
    // the single-table words are what they were: own-bucket masks and origin-bucket masks
    for (uint32_t k = 0; k < MV_NB; ++k) {
      uint32_t m = 0;
      for (uint32_t j = 0; j < sg; ++j) m |= (uint32_t)(obkt[s0 + j] >= k) << j;
      CHECK(t[GT_OWN + k] == m);
    }
    uint32_t ob = 0;
    for (uint32_t i = 0; i < t[GT_NOBS]; ++i) {
      CHECK((t[GT_OBM + i] & ob) == 0);
      ob |= t[GT_OBM + i];
    }
    CHECK(ob == all);
  }
  CHECK(seed_at == seeds.size());
  return 0;
}

int main() {
  const uint32_t N = 300;
  std::vector<uint8_t> bucket(N);
  for (uint32_t v = 0; v < N; ++v) bucket[v] = (uint8_t)((v * 7u) % MV_NB);
  // four tables of eight slots; an origin repeated inside a table (slots 0, 1), the same origin
  // in two tables (slots 2 and 9), the same origin on both sides of the group boundary in the
  // straddling table (slots 25 and 29)
  std::vector<uint32_t> origins(32), stab(32);
  for (uint32_t o = 0; o < 32; ++o) { origins[o] = 10 + 9 * o; stab[o] = o / 8; }
  origins[1] = origins[0];
  origins[9] = origins[2];
  origins[29] = origins[25];
  if (check(32, 28, origins, bucket, &stab)) return 1;
  {  // the straddling table appears in both groups; its seeds are split at the boundary
    std::vector<uint8_t> obkt(32);
    for (uint32_t o = 0; o < 32; ++o) obkt[o] = bucket[origins[o]];
    std::vector<uint32_t> gtab;
    std::vector<MvSeed> seeds;
    std::vector<MvGroup> groups;
    mv_groups_build(32, 28, origins.data(), obkt.data(), bucket.data(), stab.data(), gtab, seeds, groups);
    const uint32_t *t0 = gtab.data(), *t1 = gtab.data() + GT_STRIDE;
    CHECK(t0[GT_NT] == 4 && t1[GT_NT] == 1);
    CHECK(t0[GT_TI + 3] == 3 && t0[GT_TM + 3] == 0x0F000000u);  // slots 24..27
    CHECK(t1[GT_TI + 0] == 3 && t1[GT_TM + 0] == 0xFu);         // slots 28..31
    CHECK(t0[GT_TM + 0] == 0xFFu && t0[GT_TM + 1] == 0xFF00u && t0[GT_TM + 2] == 0xFF0000u);
    // group 0: 28 slots, origins 0 = 1 share a seed (same table), 2 and 9 do not (two tables)
    CHECK(groups[0].nseed == 27 && groups[1].nseed == 4);
    CHECK(seeds[0].y == 0x3u);
    uint32_t with2 = 0;
    for (uint32_t i = 0; i < groups[0].nseed; ++i)
      if ((seeds[i].x & 0xFFFFFFu) == origins[2]) { ++with2; CHECK(seeds[i].y == 0x4u || seeds[i].y == 0x200u); }
    CHECK(with2 == 2);
  }
  // one-slot tables, narrow groups (GW = 4), a last group of one slot
  {
    std::vector<uint32_t> o2(9), s2(9);
    for (uint32_t o = 0; o < 9; ++o) { o2[o] = 5; s2[o] = o; }  // one origin, nine tables: nine seeds
    if (check(9, 4, o2, bucket, &s2)) return 1;
  }
  // one table (stab null): the table words hold table 0 with every slot, seeds per distinct origin
  if (check(32, 28, origins, bucket, nullptr)) return 1;
  std::puts("ok");
  return 0;
}
