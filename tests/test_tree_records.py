"""Delivery tree from the step-wise round's inbound records (gs_tree_enable_records):
the parents and relay load of every recorded round against the oracle's own tree (Sim.mst), in
lockstep round by round, on the level BFS (slot-major masks) and the multi-source BFS (node-major
masks; the persistent BFS feeds it). Exact equality throughout."""
import numpy as np
import pytest

import degenerate_case as dc
import engine_bind as eb
import oracle_bind as ob

gs = eb.gs
pytestmark = pytest.mark.gpu
SEED, THR, MI, ROUNDS = 11, 0.15, 2, 24
NONE = 0xFFFFFFFF
SCAN_B = 256  # k_trr_scan's block width: a level above twice it has block totals and a cross-block prefix

# tables: (active-set size, rotation probability); slots: (table, origin stake rank, fanout)
CASES = {
    # N - 1 <= active-set size: entries shorter than the ring
    "tiny7": dict(n=7, tables=[(12, .1)], slots=[(0, 1, 6), (0, 5, 6)]),
    # fanout = ring = 32: take indices up to 31, the top bit of cmask
    "wide33": dict(n=33, tables=[(32, .1)], slots=[(0, 1, 32), (0, 20, 32)]),
    # one node more than a wave
    "wave65": dict(n=65, tables=[(12, .1)], slots=[(0, 1, 6), (0, 33, 6)]),
    # the smallest N (steps of 50) at which every slot's widest level passes 2 * SCAN_B in round 0 and
    # after the prune wave (1,000: 508 in one slot); origins spread over the stake buckets
    "scan1050": dict(n=1050, tables=[(12, .1)], slots=[(0, 1, 6), (0, 131, 6), (0, 525, 6), (0, 1049, 6)],
                     scan=True),
    # failed peers keep their take index
    "fail200": dict(n=200, tables=[(12, .1)], slots=[(0, 1, 6), (0, 50, 6)], fractions=[.3, 0.]),
    # two trajectory tables, per-slot fanouts (the multi BFS only)
    "tables300": dict(n=300, tables=[(6, .1), (12, 0.)], slots=[(0, 1, 2), (0, 9, 6), (1, 1, 6), (1, 40, 2)]),
    # the level loop and the backward subtree walk at the 253-hop limit: one node per level
    "chain253": dict(chain=253, rounds=3),
}
MODES = {"level": gs.GS_BFS_LEVEL, "multi": gs.GS_BFS_MULTI}


def setup(c, mode):
    """(engine, oracle sims, origins, tables, table of each slot, n) of a case, before the first round."""
    if "chain" in c:
        case = dc.chain_case(c["chain"])
        eng = dc.chain_engine(case, 2, bfs_mode=mode)
        origins = case["c"][:2]
        eng.set_slots(origins, MI, THR)
        return eng, [dc.chain_sim(case) for _ in origins], origins, [(dc.ASZ, 0.)], [0, 0], case["n"]
    n, slots, tables = c["n"], c["slots"], c["tables"]
    fanouts, tabs = [f for _, _, f in slots], [t for t, _, _ in slots]
    pks, st = eb.synth.network(n)
    kw = dict(active_set_size=tables[0][0], rotation_probability=tables[0][1])
    if len(tables) > 1:
        kw = dict(trajectories=[(a, p, tabs.count(t)) for t, (a, p) in enumerate(tables)], traj_multi=True)
    eng = gs.Engine(st, len(slots), fanout=max(fanouts), seed=SEED, bfs_mode=mode, **kw)
    sims = [ob.Sim(ob.PHILOX, SEED, pks, st, f) for f in fanouts]
    origins = [sims[0].find_nth_largest(r) for _, r, _ in slots]
    eng.set_slots(origins, MI, THR)
    if len(set(fanouts)) > 1:
        eng.set_slot_fanouts(fanouts)
    eng.init_active_sets()
    for s, t in zip(sims, tabs):
        s.init_philox(tables[t][0])
    if "fractions" in c:
        eng.fail_nodes(c["fractions"])
        for s, f in zip(sims, c["fractions"]):
            s.fail_nodes(f)
    return eng, sims, origins, tables, tabs, n


@pytest.mark.parametrize("name,mode", [(c, m) for c in CASES for m in MODES if c != "tables300" or m == "multi"])
def test_tree_records_match_oracle(name, mode):
    c = CASES[name]
    eng, sims, origins, tables, tabs, n = setup(c, MODES[mode])
    assert not eng.info()["fused_round"] and eng.info()["bfs_mode"] == MODES[mode]
    eng.enable_tree(records=True)
    S, rounds = len(sims), c.get("rounds", ROUNDS)
    kids, sub, prunes = np.zeros((S, n), np.uint64), np.zeros((S, n), np.uint64), 0
    for r in range(rounds):
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
            if c.get("scan") and r in (0, rounds - 1):  # (a quiet shrink of n would lose the block totals)
                assert np.bincount(level[level > 0]).max() > 2 * SCAN_B, f"slot {k} round {r}"
            if "chain" in c and k == 0:  # from the chain's head: one node per level, every subtree a suffix
                assert level.max() == c["chain"] and np.bincount(level[level > 0]).max() == 1
            s.consume_messages(o)
            s.send_prunes(o, THR, MI)
            prunes += len(s.prunes())
            s.prune_connections()
            s.chance_to_rotate(*tables[tabs[k]], r)
    assert prunes > 0 or "chain" in c  # (the masks were not idle)
    for k in range(S):
        ch, sb, cnt = eng.tree_load(k)
        np.testing.assert_array_equal(ch, kids[k], err_msg=f"slot {k}")
        np.testing.assert_array_equal(sb, sub[k], err_msg=f"slot {k}")
        assert cnt == rounds
    ch, sb, cnt = eng.tree_load()
    np.testing.assert_array_equal(ch, kids.sum(axis=0))
    np.testing.assert_array_equal(sb, sub.sum(axis=0))
    assert cnt == rounds
    eng.close()


def test_tree_records_refusals_and_disable():
    pks, st = eb.synth.network(150)

    def make(mode, p=.1):
        e = gs.Engine(st, 3, seed=SEED, rotation_probability=p, bfs_mode=mode)
        e.set_slots([1, 40, 90], MI, THR)
        e.init_active_sets()
        return e

    wg, a, twin, still = make(gs.GS_BFS_WORKGROUP), make(gs.GS_BFS_MULTI), make(gs.GS_BFS_MULTI), make(gs.GS_BFS_LEVEL, 0.)
    assert wg.info()["fused_round"]
    for call in (lambda: wg.enable_tree(records=True), lambda: a.enable_tree(), lambda: a.tree(0)):
        with pytest.raises(gs.GsError) as ei:  # the one-kernel round; not the one-kernel round; not enabled
            call()
        assert ei.value.code == -5
    a.round(0, record=False)  # (the multi BFS allocates its inbound rows on the first round)
    twin.round(0, record=False)
    before = a.info()["pair_bytes"]
    a.enable_tree(records=True)
    a.enable_tree(records=True)  # (a no-op)
    assert a.info()["pair_bytes"] == before + 36 * 3 * 150  # 12 B of results + 24 B of scratch per pair
    a.round(1, record=False)
    with pytest.raises(gs.GsError) as ei:  # no recorded round yet
        a.tree(0)
    assert ei.value.code == -5
    for r in range(2, 8):
        a.round(r, record=True)
    assert a.tree_load()[2] == 6 and (a.tree(1) != NONE).any()
    a.enable_tree(False)
    assert a.info()["pair_bytes"] == before
    for r in range(1, 8):
        twin.round(r, record=r >= 2)
    for e in (a, twin):
        e.round(8, record=True)
    for k in range(3):
        np.testing.assert_array_equal(a.hops(k), twin.hops(k))
        for x, y in zip(a.caches(k), twin.caches(k)):
            np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(a.summaries(), twin.summaries())
    # gs_read_mst applies after a round that changed neither rows nor masks (no rotation; round 0 prunes nothing)
    still.enable_tree(records=True)
    still.round(0, record=True)
    for k in range(3):
        assert still.mst(k) == still.tree_children(k)
    for e in (wg, a, twin, still):
        e.close()
