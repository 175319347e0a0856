"""The one-kernel round's sort-free consume (gs_round_wg.hip, consume_lane).

The lane path keeps only the two smallest (hop, id) records by a running min/max and
appends the other absent ids in record order, so the physical row order of a cache
entry differs from the sorted-record algorithms'; the entry as a map must not. A round
that the 50-key limit would cut short goes to the wave path, which ranks its records.
Everything here is bit-exact: against the split-round engine (step kernels, which rank
every record) and against the oracle.
"""
import numpy as np
import pytest

import engine_bind as eb
import oracle_bind as ob

gs = eb.gs
pytestmark = pytest.mark.gpu
U64MAX = np.uint64(2**64 - 1)
THR, MI = 0.15, 2
CHECK_ROUNDS = (1, 18, 19, 20, 39, 40, 44)  # two prune waves (upserts reach 20 at rounds 19 and 39)


def spread_origins(st, S):
    """S origins spread over the stake order, so the slots use different entry buckets."""
    order = np.argsort(np.asarray(st, dtype=np.uint64), kind="stable")
    return [int(order[(k * (len(order) - 1)) // (S - 1)]) for k in range(S)]


def assert_same_state(a, b, slots, tag):
    for k in slots:
        np.testing.assert_array_equal(a.hops(k), b.hops(k), err_msg=f"hops slot {k} {tag}")
        np.testing.assert_array_equal(a.pruned_all(k), b.pruned_all(k), err_msg=f"prune state slot {k} {tag}")
        for name, x, y in zip(("upserts", "len", "keys", "scores"), a.caches(k), b.caches(k)):
            np.testing.assert_array_equal(x, y, err_msg=f"cache {name} slot {k} {tag}")
        for x, y in zip(a.accumulators(k), b.accumulators(k)):
            np.testing.assert_array_equal(x, y, err_msg=f"accumulators slot {k} {tag}")


def assert_oracle_caches(eng, k, sim, origin, tag):
    up, ln, keys, sc = eng.caches(k)
    oup, oln, okeys, osc = sim.caches(origin)
    has = oup != 0xFFFFFFFF
    np.testing.assert_array_equal(up[has], oup[has], err_msg=f"upserts {tag}")
    np.testing.assert_array_equal(ln, oln, err_msg=f"len {tag}")
    np.testing.assert_array_equal(keys, okeys, err_msg=f"keys {tag}")
    np.testing.assert_array_equal(sc, osc, err_msg=f"scores {tag}")


def engine_pair(st, S, origins, *, p, seed, fanout=6, asz=12):
    engines = [gs.Engine(st, S, seed=seed, fanout=fanout, active_set_size=asz, rotation_probability=p,
                         bfs_mode=gs.GS_BFS_WORKGROUP, split_round=f) for f in (False, True)]
    assert engines[0].info()["fused_round"] and not engines[1].info()["fused_round"]
    for e in engines:
        e.set_slots(origins, MI, THR)
        e.init_active_sets()
    return engines


@pytest.mark.parametrize("n,S,with_oracle", [(300, 12, True), (600, 9, False)])
def test_fused_matches_split_and_oracle(n, S, with_oracle):
    """45 rounds at rotation probability 0.05 through two prune waves: the one-kernel round ==
    the split round at the rounds around each wave (every slot), and, at n = 300, == the oracle
    round by round on two slots."""
    seed, p = 23, 0.05
    pks, st = eb.synth.network(n)
    origins = spread_origins(st, S)
    fused, split = engine_pair(st, S, origins, p=p, seed=seed)
    sims = {k: ob.Sim(ob.PHILOX, seed, pks, st, 6) for k in ((0, S - 1) if with_oracle else ())}
    for s in sims.values():
        s.init_philox(12)
    prunes = 0
    for r in range(45):
        fused.round(r, record=r >= 5)
        split.round(r, record=r >= 5)
        if r in CHECK_ROUNDS:
            assert_same_state(fused, split, range(S), f"round {r}")
        for k, s in sims.items():
            o = origins[k]
            s.run_gossip(o)
            s.consume_messages(o)
            s.send_prunes(o, THR, MI)
            np.testing.assert_array_equal(fused.distances(k), s.distances(), err_msg=f"hops slot {k} round {r}")
            assert fused.prunes(k) == s.prunes(), f"prunes slot {k} round {r}"
            prunes += len(s.prunes())
            s.prune_connections()
            if r in CHECK_ROUNDS:
                assert_oracle_caches(fused, k, s, o, f"slot {k} round {r}")
            s.chance_to_rotate(12, p, r)
            if r in CHECK_ROUNDS:
                np.testing.assert_array_equal(fused.pruned_all(k), s.pruned_all(o), err_msg=f"prune state {k} {r}")
    np.testing.assert_array_equal(fused.summaries(), split.summaries())
    assert int(fused.summaries()["prunes"].sum()) > 0
    assert not with_oracle or prunes > 0
    for e in (fused, split):
        e.close()


def test_state_changes_between_fused_rounds():
    """fail_nodes before round 7, per-slot fanouts before round 11 and one step-wise round at 15,
    each between one-kernel rounds: still equal to the split round's step kernels."""
    n, S, seed, p = 300, 12, 29, 0.05
    pks, st = eb.synth.network(n)
    origins = spread_origins(st, S)
    engines = engine_pair(st, S, origins, p=p, seed=seed)
    for r in range(45):
        for e in engines:
            if r == 7:
                e.fail_nodes([0.1] * S)
            if r == 11:
                e.set_slot_fanouts([6 - k % 3 for k in range(S)])
            if r == 15:
                e.run_gossip()
                e.consume_messages()
                e.send_prunes()
                e.prune_connections()
                e.chance_to_rotate(r)
                e.record_round()
            else:
                e.round(r, record=r >= 5)
        if r in (7, 8, 11, 12, 15, 16) + CHECK_ROUNDS:
            assert_same_state(engines[0], engines[1], range(S), f"round {r}")
    np.testing.assert_array_equal(engines[0].summaries(), engines[1].summaries())
    for e in engines:
        e.close()


def cut_short_nodes(sim, origin, near):
    """From the oracle's own state between run_gossip and consume_messages: the nodes among
    `near` with 1 <= c <= 16 records this round whose insertions ReceivedCache::record cuts
    short -- lt < 50 and lt + n > 50, with lt = the entry's length plus the timely records
    (the two smallest by (hop, id)) it lacks and n = the other records it lacks. Returns
    {node: (c, len, lt, n)}."""
    out = {}
    for v in near:
        rec = sim.orders(int(v)) or []
        if not 1 <= len(rec) <= 16:
            continue
        ent = sim.cache(int(v), origin)
        keys = set(ent[1]) if ent else set()
        rec = sorted(rec, key=lambda x: (x[1], x[0]))
        lt = len(keys) + sum(1 for src, _ in rec[:2] if src not in keys)
        nn = sum(1 for src, _ in rec[2:] if src not in keys)
        if lt < 50 and lt + nn > 50:
            out[int(v)] = (len(rec), len(keys), lt, nn)
    return out


def run_limit_case(n, fanout, asz, origins, rounds, *, fail_at=None, fraction=0.0, seed=11):
    """Rotation probability 1: every node's pushers turn over each round, so entries grow
    towards ReceivedCacheEntry::CAPACITY = 50 before their 20th upsert. The fused engine's
    caches are compared with the oracle's after every round. Returns reached: per (slot, round,
    node) whose oracle entry reached 50 keys in that round, its in-degree in that round; and
    cut: per (slot, round), cut_short_nodes of that round when there are any."""
    pks, st = eb.synth.network(n)
    S = len(origins)
    eng = gs.Engine(st, S, seed=seed, fanout=fanout, active_set_size=asz, rotation_probability=1.0,
                    bfs_mode=gs.GS_BFS_WORKGROUP)
    assert eng.info()["fused_round"]
    eng.set_slots(origins, MI, THR)
    eng.init_active_sets()
    sims = [ob.Sim(ob.PHILOX, seed, pks, st, fanout) for _ in origins]
    for s in sims:
        s.init_philox(asz)
    prev = [np.zeros(n, dtype=np.uint32) for _ in origins]
    reached, cut = {}, {}
    for r in range(rounds):
        if r == fail_at:
            eng.fail_nodes([fraction] * S)
            for s in sims:
                s.fail_nodes(fraction)
        eng.round(r)
        for k, (s, o) in enumerate(zip(sims, origins)):
            s.run_gossip(o)
            c = cut_short_nodes(s, o, np.nonzero(prev[k] >= 34)[0])  # (a round adds 16 keys at most)
            if c:
                cut[(k, r)] = c
            s.consume_messages(o)
            s.send_prunes(o, THR, MI)
            assert eng.prunes(k) == s.prunes(), f"prunes slot {k} round {r}"
            s.prune_connections()
            indeg = s.counters()[1]
            assert_oracle_caches(eng, k, s, o, f"slot {k} round {r}")
            ln = s.caches(o)[1]
            for v in np.nonzero((ln >= 50) & (prev[k] < 50))[0]:
                reached[(k, r, int(v))] = int(indeg[v]) if indeg[v] != U64MAX else 0
            prev[k] = ln.copy()
            s.chance_to_rotate(asz, 1.0, r)
    eng.close()
    return reached, cut


def test_cache_limit_of_50_keys():
    """200 nodes, fanout = active set = 20, rotation probability 1: the oracle's own lengths
    show an entry at the 50-key limit (round 15 for origin 0, 17 for origin 7; chosen with the
    oracle on the CPU); caches equal the oracle's every round up to two rounds past it."""
    reached, _ = run_limit_case(200, 20, 20, [0, 7], 20)
    assert reached, "no oracle entry reached 50 keys: the case tests nothing"
    for k in (0, 1):  # both slots, and two more compared rounds after each slot's first
        assert min(r for kk, r, _ in reached if kk == k) + 2 <= 19


@pytest.mark.parametrize("n,fanout,origins,fraction,rounds", [
    (400, 20, [3, 18], 0.5, 21),  # node 306, round 18: 15 records, 48 keys, 3 more absent (both slots)
    (300, 28, [12, 27], 0.6, 22),  # round 17: node 69 (slot 0, 12 records) and node 43 (slot 1, 9 records),
                                   # 49 keys and 2 more absent; slot 1 again in round 19, node 253, 16 records
])
def test_limit_cuts_a_register_path_round_short(n, fanout, origins, fraction, rounds):
    """The register consume path's fallback: a node with 1 <= c <= 16 records whose entry has
    room for some but not all of the round's absent non-timely records (lt < 50 < lt + n), so
    rank order decides which get in: consume_lane stores nothing and the wave path takes the
    node. Half (or 60 %) of the nodes fail before round 15, which brings in-degrees under 16
    while the entries are near the limit. The condition is asserted from the oracle's records
    and entry before that round's consume (cases chosen with the oracle on the CPU); caches
    equal the oracle's every round through it and two rounds past it."""
    _, cut = run_limit_case(n, fanout, fanout, origins, rounds, fail_at=15, fraction=fraction)
    for k in range(len(origins)):
        hit = [r for kk, r in cut if kk == k]
        assert hit, f"slot {k}: no round was cut short on a node of in-degree <= 16: the case tests nothing"
        assert min(hit) + 2 <= rounds - 1, f"slot {k}: first cut round {min(hit)} leaves no two compared rounds after it"
