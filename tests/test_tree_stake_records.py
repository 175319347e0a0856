"""The records mode of the delivery tree in stake (gs_tree_stake_enable_records): the
level walk over the records tree's queue, exactly equal to test_tree_stake.py's Python-int
expectation (built from Engine.tree, Engine.hops and the stakes after each recorded round)."""
import os
import re

import numpy as np
import pytest

import degenerate_case as dc
import test_cluster_view as tv
import test_tree_stake as ts
from test_cluster_groups import raises

gs, synth = tv.gs, tv.synth
gpu = pytest.mark.gpu
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gossip_hip.h")
MODES = [gs.GS_BFS_LEVEL, gs.GS_BFS_MULTI]
THIN = 256  # a level wider than this in some slot takes a launch of its own


def test_symbol_declared_and_bound():
    with open(HEADER) as f:
        assert re.search(r"^int gs_tree_stake_enable_records\(gs_engine\* e,", f.read(), re.M)
    assert "gs_tree_stake_enable_records" in gs.EXPORTS


def engine(bfs, st, s, **kw):
    return gs.Engine(st, s, bfs_mode=bfs, **{**dict(seed=23, active_set_size=12, rotation_probability=0.1), **kw})


def drive(eng, st, origins, rounds, groups=None, weights=None, *, fractions=None, init=True, tag=""):
    s = len(origins)
    ex = ts.Expect(st, groups or [s], weights or [1] * s)
    eng.set_slots(origins, 2, 0.15)
    if init:
        eng.init_active_sets()
    eng.enable_tree(records=True)
    eng.enable_tree_stake(groups=groups, weights=weights, records=True)
    if fractions:
        eng.fail_nodes(fractions)
    for r in range(rounds):
        eng.round(r, record=True)
        ex.record(eng, f"{tag} round {r}")
        ex.check(eng, f"{tag} round {r}")
    return ex


@gpu
@pytest.mark.parametrize("bfs", MODES)
@pytest.mark.parametrize("case", ["tiny7", "groups131", "trips1050"])
def test_records_walk_matches_python(case, bfs):
    if case == "tiny7":  # a level is narrower than a wave
        st = synth.network(7)[1]
        eng = engine(bfs, st, 2)
        ex = drive(eng, st, [1, 5], 6, tag=case)
    elif case == "groups131":  # the chunk table, a skipped slot, unreached nodes; every level thin
        st = synth.network(tv.N1)[1]
        eng = engine(bfs, st, tv.S1)
        ex = drive(eng, st, tv.ORIGINS1, 8, [3, 1, 3], [1, 2, 0, 5, 1, 1, 3], fractions=[0.3] * tv.S1, tag=case)
        assert ex.unreached > 0, "every node was reached"
    else:  # a wide level with full sibling runs, thin runs on both sides of it
        st = synth.network(1050)[1]
        eng = engine(bfs, st, 4, seed=11, fanout=6)
        ex = drive(eng, st, ts.by_stake_rank(st, (1, 131, 525, 1049)), 3, tag=case)
        assert ex.widest > THIN, "no level wider than the thin kernel's workgroup"
    assert ex.rounds > 0 and sum(ex.tot[0]["subtree"]) > 0
    eng.close()


@gpu
@pytest.mark.parametrize("bfs", MODES)
def test_chain_253_levels_one_walk_launch(bfs):
    case, rounds = dc.chain_case(253), 3
    eng = dc.chain_engine(case, 2, bfs_mode=bfs, profile=True)
    ex = drive(eng, case["stakes"], case["c"][:2], rounds, init=False, tag="chain")
    head = case["c"][0]  # from the chain's head every subtree is a suffix of the chain
    assert ex.last[0]["subtree"][head] >= 253 and ex.last[0]["below"][head] >= 253 * dc.STAKE and ex.widest <= 2
    assert eng.kernel_time("tree_stake")[1] == 4 * rounds  # every level is thin: the walk is one launch
    eng.close()


@gpu
@pytest.mark.parametrize("bfs", MODES)
def test_past_both_old_bounds(bfs):
    n, s = 70_000, 2
    st = synth.network(n)[1]
    eng = engine(bfs, st, s, seed=5)
    eng.enable_tree(records=True)
    raises(ts.GS_ERANGE, eng.enable_tree_stake, "10175 nodes")
    ex = drive(eng, st, [3, 40_000], 1, [1, 1], tag="n70000")
    assert max(ex.last[0]["subtree"]) >= 2**16  # (slot 0's origin: a 16-bit pack or node id fails here)
    eng.close()


@gpu
def test_lifecycle(monkeypatch):
    n, s, E = tv.N1, tv.S1, ts.GS_ESTATE
    eng, wg = tv.engine1(monkeypatch, "level"), tv.engine1(monkeypatch, "wg_fused")
    for e in (eng, wg):
        e.set_slots(tv.ORIGINS1)
    raises(E, lambda: eng.enable_tree_stake(records=True), "gs_tree_enable_records")  # no tree at all
    wg.enable_tree()
    raises(E, lambda: wg.enable_tree_stake(records=True), "gs_tree_enable_records")  # the one-kernel tree
    wg.close()
    eng.enable_tree(records=True)
    b0 = ts.sizes(eng)
    eng.enable_tree_stake(records=True)
    eng.enable_tree_stake(records=True)  # twice: a no-op
    assert ts.sizes(eng)["pair_bytes"] - b0["pair_bytes"] == 12 * s * n
    raises(E, eng.enable_tree_stake)  # each kind refuses while the other is on
    eng.enable_tree_stake(False)
    assert ts.sizes(eng) == b0
    eng.enable_tree_stake()
    raises(E, lambda: eng.enable_tree_stake(records=True))
    eng.enable_tree_stake(False)
    assert ts.sizes(eng) == b0
    eng.close()
