"""Delivery tree on the device (gs_tree_enable): k_tree_wg's first-discoverer parents
and relay load of every recorded one-kernel round against the oracle's own tree (Sim.mst: the
nodes each node first discovered in the last run_gossip), run in lockstep round by round.
Exact equality throughout."""
import numpy as np
import pytest

import engine_bind as eb
import oracle_bind as ob

gs = eb.gs
pytestmark = pytest.mark.gpu
SEED, THR, MI, ROUNDS = 11, 0.15, 2, 24
NONE = 0xFFFFFFFF
TREE_THREADS = 512  # k_tree_wg's workgroup: a level above it takes several trips

# tables: (active-set size, rotation probability); slots: (table, origin stake rank, fanout)
CASES = {
    # N - 1 <= active-set size: short entries
    "tiny7": dict(n=7, tables=[(12, .1)], slots=[(0, 1, 6), (0, 5, 6)]),
    # fanout = ring = 32: the widest push columns
    "wide33": dict(n=33, tables=[(32, .1)], slots=[(0, 1, 32), (0, 20, 32)]),
    # one node more than a wave
    "wave65": dict(n=65, tables=[(12, .1)], slots=[(0, 1, 6), (0, 33, 6)]),
    # the smallest N (steps of 50) at which every slot's widest level passes the workgroup in round 0
    # and after the prune wave (1,000: 508 in one slot): cross-wave prefix and cross-trip base;
    # origins spread over the stake buckets
    "trips1050": dict(n=1050, tables=[(12, .1)], slots=[(0, 1, 6), (0, 131, 6), (0, 525, 6), (0, 1049, 6)],
                      trips=True),
    # failed peers burn take slots
    "fail200": dict(n=200, tables=[(12, .1)], slots=[(0, 1, 6), (0, 50, 6)], fractions=[.3, 0.]),
    # two trajectory tables, per-slot fanouts
    "tables300": dict(n=300, tables=[(6, .1), (12, 0.)], slots=[(0, 1, 2), (0, 9, 6), (1, 1, 6), (1, 40, 2)]),
}


@pytest.mark.parametrize("name", list(CASES))
def test_tree_matches_oracle(name):
    c = CASES[name]
    n, slots, tables = c["n"], c["slots"], c["tables"]
    S, fanouts, tabs = len(slots), [f for _, _, f in slots], [t for t, _, _ in slots]
    pks, st = eb.synth.network(n)
    kw = dict(active_set_size=tables[0][0], rotation_probability=tables[0][1])
    if len(tables) > 1:
        kw = dict(trajectories=[(a, p, tabs.count(t)) for t, (a, p) in enumerate(tables)])
    eng = gs.Engine(st, S, fanout=max(fanouts), seed=SEED, bfs_mode=gs.GS_BFS_WORKGROUP, **kw)
    assert eng.info()["fused_round"]
    sims = [ob.Sim(ob.PHILOX, SEED, pks, st, f) for f in fanouts]
    origins = [sims[0].find_nth_largest(r) for _, r, _ in slots]
    eng.set_slots(origins, MI, THR)
    if len(set(fanouts)) > 1:
        eng.set_slot_fanouts(fanouts)
    eng.init_active_sets()
    eng.enable_tree()
    for s, t in zip(sims, tabs):
        s.init_philox(tables[t][0])
    if "fractions" in c:
        eng.fail_nodes(c["fractions"])
        for s, f in zip(sims, c["fractions"]):
            s.fail_nodes(f)
    kids, sub, prunes = np.zeros((S, n), np.uint64), np.zeros((S, n), np.uint64), 0
    for r in range(ROUNDS):
        eng.round(r, record=True)
        for k, (s, o) in enumerate(zip(sims, origins)):
            s.run_gossip(o)
            want = {u: sorted(m) for u in range(n) for m in [s.mst(u)] if m}
            assert eng.tree_children(k) == want, f"slot {k} round {r}"
            parent, hops = eng.tree(k), eng.hops(k).astype(np.int64)
            reached = parent != NONE
            np.testing.assert_array_equal(reached, (hops != 0xFF) & (np.arange(n) != o), err_msg=f"slot {k} round {r}")
            np.testing.assert_array_equal(hops[parent[reached]] + 1, hops[reached], err_msg=f"slot {k} round {r}")
            # the round's child counts and subtree sizes from the oracle's tree, deepest level first
            par, dist = np.zeros(n, np.int64), s.distances()
            for u, ws in want.items():
                par[ws] = u
                kids[k, u] += len(ws)
            level = np.where(dist == np.uint64(2**64 - 1), 0, dist).astype(np.int64)
            below = np.zeros(n, np.uint64)
            for d in range(int(level.max()), 0, -1):
                w = np.nonzero(level == d)[0]
                np.add.at(below, par[w], below[w] + np.uint64(1))
            sub[k] += below
            if c.get("trips") and r in (0, ROUNDS - 1):  # (a quiet shrink of n would lose the trips)
                assert np.bincount(level[level > 0]).max() > TREE_THREADS, f"slot {k} round {r}"
            s.consume_messages(o)
            s.send_prunes(o, THR, MI)
            prunes += len(s.prunes())
            s.prune_connections()
            s.chance_to_rotate(*tables[tabs[k]], r)
    assert prunes > 0  # (the masks were not idle)
    for k in range(S):
        ch, sb, rounds = eng.tree_load(k)
        np.testing.assert_array_equal(ch, kids[k], err_msg=f"slot {k}")
        np.testing.assert_array_equal(sb, sub[k], err_msg=f"slot {k}")
        assert rounds == ROUNDS
    ch, sb, rounds = eng.tree_load()
    np.testing.assert_array_equal(ch, kids.sum(axis=0))
    np.testing.assert_array_equal(sb, sub.sum(axis=0))
    assert rounds == ROUNDS
    eng.close()


def test_tree_refusals_and_disable(monkeypatch):
    monkeypatch.setenv("GS_ROUND_SPLIT", "force")
    pks, st = eb.synth.network(150)

    def make(mode):
        e = gs.Engine(st, 3, seed=SEED, rotation_probability=.1, bfs_mode=mode)
        e.set_slots([1, 40, 90], MI, THR)
        e.init_active_sets()
        return e

    a, twin, multi = make(gs.GS_BFS_WORKGROUP), make(gs.GS_BFS_WORKGROUP), make(gs.GS_BFS_MULTI)
    for call in (lambda: a.tree(0), lambda: a.tree_load(0), lambda: multi.enable_tree()):
        with pytest.raises(gs.GsError) as ei:  # not enabled; not the one-kernel round
            call()
        assert ei.value.code == -5
    assert a.info()["round_split"]
    before = a.info()["pair_bytes"]
    a.enable_tree()
    a.enable_tree()  # (a no-op)
    assert not a.info()["round_split"] and a.info()["pair_bytes"] == before + 12 * 3 * 150
    a.round(0, record=False)
    with pytest.raises(gs.GsError) as ei:  # no recorded round yet
        a.tree(0)
    assert ei.value.code == -5
    for r in range(1, 8):
        a.round(r, record=True)
    assert a.tree_load()[2] == 7 and (a.tree(1) != NONE).any()
    a.enable_tree(False)
    assert a.info()["round_split"] and a.info()["pair_bytes"] == before
    for r in range(8):
        twin.round(r, record=r >= 1)
    for e in (a, twin):
        e.round(8, record=True)
    for k in range(3):
        np.testing.assert_array_equal(a.hops(k), twin.hops(k))
        for x, y in zip(a.caches(k), twin.caches(k)):
            np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(a.summaries(), twin.summaries())
    for e in (a, twin, multi):
        e.close()
