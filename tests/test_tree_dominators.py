"""Delivery dominators (gs_tree_stake_enable_dominators), exactly equal to a reference in
plain Python over what the engine returns after the round: Engine.inbound(slot), Engine.hops(slot)
and the stakes. Dominator SETS by the textbook iteration Dom(w) = {w} | intersection of Dom(src)
over w's recorded sources, to a fixpoint (a set not computed yet stands for "every node"); idom is
the strict dominator of largest hop; below / kids / sub are Python ints. test_tree_stake.Expect
holds the grouping, the weights and the comparison of the group reads."""
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
NONE = ts.NONE


def test_symbols_declared_and_bound():
    with open(HEADER) as f:
        text = f.read()
    for name in ("gs_tree_stake_enable_dominators", "gs_read_dominators"):
        assert re.search(r"^int %s\(gs_engine\* e," % name, text, re.M), name
        assert name in gs.EXPORTS
    with pytest.raises(ValueError):  # refused before any engine call
        gs.Engine.enable_tree_stake(None, dominators=True)


def reference(eng, j, origin):
    """(idom[n], {w: Dom(w)}) of slot j's last round."""
    n, hops = eng.n, eng.hops(j).tolist()
    off, src, _ = eng.inbound(j)
    order = sorted((w for w in range(n) if hops[w] != 255 and w != origin), key=lambda w: (hops[w], w))
    pred = {w: [s for s in src[off[w]:off[w + 1]].tolist() if s < n and hops[s] != 255] for w in order}
    dom, changed = {origin: {origin}}, True
    while changed:
        changed = False
        for w in order:
            new = set.intersection(*[dom[s] for s in pred[w] if s in dom]) | {w}
            if dom.get(w) != new:
                dom[w], changed = new, True
    idom = [NONE] * n
    for w in order:
        idom[w] = max(dom[w] - {w}, key=lambda v: hops[v])
    return idom, dom


class Expect(ts.Expect):
    """ts.Expect with the dominator tree's per-slot quantities; odd / same count, on the reference,
    the nodes whose idom is neither their first-delivery parent nor the origin / is that parent."""
    odd = same = moved = 0

    def record(self, eng, origins, what=""):
        n, self.last, j0 = len(self.st), [], 0
        for g, ns in enumerate(self.groups):
            last = {k: [0] * n for k in ts.KEYS}
            for j in range(j0, j0 + ns):
                idom, dom = reference(eng, j, origins[j])
                assert eng.dominators(j).tolist() == idom, f"{what}: slot {j} idom"
                kids, sub, below = [0] * n, [0] * n, [0] * n
                for w, ds in dom.items():
                    for v in ds - {w}:
                        sub[v], below[v] = sub[v] + 1, below[v] + self.st[w]
                    if w != origins[j]:
                        kids[idom[w]] += 1
                assert [int(x) for x in eng.tree_stake(j)] == below, f"{what}: slot {j} below"
                for w, p in enumerate(eng.tree(j).tolist()):
                    self.odd += idom[w] not in (NONE, p, origins[j])
                    self.same += idom[w] == p != NONE
                    self.moved += idom[w] != p
                for k, a in zip(ts.KEYS, (kids, sub, below)):
                    last[k] = [x + self.w[j] * y for x, y in zip(last[k], a)]
            j0 += ns
            for k in ts.KEYS:
                self.tot[g][k] = [x + y for x, y in zip(self.tot[g][k], last[k])]
            self.last.append(last)
        self.rounds += 1


def drive(eng, st, origins, rounds, groups=None, weights=None, *, fractions=None, init=True, tag=""):
    s = len(origins)
    ex = Expect(st, groups or [s], weights or [1] * s)
    eng.set_slots(origins, 2, 0.15)
    if init:
        eng.init_active_sets()
    eng.enable_tree(records=True)
    eng.enable_tree_stake(groups=groups, weights=weights, records=True, dominators=True)
    if fractions:
        eng.fail_nodes(fractions)
    for r in range(rounds):
        eng.round(r, record=True)
        ex.record(eng, origins, f"{tag} round {r}")
        ex.check(eng, f"{tag} round {r}")  # (the sums over the rounds are the sums of the per-round values)
    return ex


# n, push fanout of each slot, seed, rounds, groups, weights, failed fraction: 4 origins each. Seeds
# and fanouts chosen so that the reference alone meets the asserts on ex.odd and ex.same (with
# fanout 6 everywhere the origin dominates nearly every node).
CASES = {
    "tiny7": (7, [2] * 4, 58, 4, None, None, None),  # fewer nodes than a wave
    "groups131": (131, [2] * 4, 23, 3, [2, 2], [1, 1, 3, 3], None),  # every level thin; two weighted groups
    "failed131": (131, [3] * 4, 7, 3, [1, 3], [2, 0, 1, 3], 0.3),  # unreached nodes, a slot of weight 0
    "wide1050": (1050, [2, 2, 6, 6], 7, 2, None, None, None),  # levels above two blocks of 256: the wide kernels
}


@gpu
@pytest.mark.parametrize("bfs", MODES)
@pytest.mark.parametrize("case", list(CASES))
def test_dominators_match_python(case, bfs):
    n, fanouts, seed, rounds, groups, weights, frac = CASES[case]
    st = synth.network(n)[1]
    eng = gs.Engine(st, 4, bfs_mode=bfs, seed=seed, fanout=max(fanouts), active_set_size=12, rotation_probability=0.1)
    eng.set_slot_fanouts(fanouts)
    origins = [1, 5, 3, 6] if n == 7 else ts.by_stake_rank(st, (1, n // 8, n // 2, n - 1))
    ex = drive(eng, st, origins, rounds, groups, weights, fractions=[frac] * 4 if frac else None, tag=case)
    assert ex.odd > 0, "no node whose dominator is neither its first-delivery parent nor the origin"
    assert ex.same > 0, "no node whose dominator is its first-delivery parent"
    if frac:
        assert NONE in eng.dominators(0).tolist()[1:] and 255 in eng.hops(0).tolist(), "every node was reached"
    if n == 1050:
        assert max(max(np.bincount(eng.hops(j))[1:254]) for j in (2, 3)) > 512, "no level wider than two of the wide kernels' blocks"
    eng.close()


def launches_per_round(sweeps):
    """Every level thin: the init, one launch per sweep, the two walks, the reduce and the fold."""
    return 1 + sweeps + 2 + 2


@gpu
@pytest.mark.parametrize("bfs", MODES)
def test_cascade_takes_several_sweeps(bfs):
    """o -> c1 .. c7, a side chain o -> s1 .. s8 -> c6, and pushes back up: c7 -> c5, c5 -> a5 -> c4,
    c4 -> a4 -> c3. c6 hears from both chains, so idom[c6] = o at once; z1 = c5 hears from c4 and
    from c7 below c6, z2 = c4 from c3 and from a5 below c5, z3 = c3 from c2 and from a4 below c4:
    each finds the origin only once the one before has moved, and levels go shallowest first."""
    names = ["o"] + [f"c{i}" for i in range(1, 8)] + [f"s{i}" for i in range(1, 9)] + ["a5", "a4"]
    ids = dict(zip(names, np.random.default_rng(3).permutation(len(names) + 6).tolist()))
    edges = {"o": ["c1", "s1"], "c7": ["c5"], "c5": ["c6", "a5"], "a5": ["c4"], "c4": ["c5", "a4"], "a4": ["c3"],
             "s8": ["c6"]}
    for i in (1, 2, 3, 6):
        edges[f"c{i}"] = [f"c{i + 1}"]
    for i in range(1, 8):
        edges[f"s{i}"] = [f"s{i + 1}"]
    stakes = np.full(len(names) + 6, dc.STAKE, dtype=np.uint64)
    eng = gs.Engine(stakes, 1, fanout=dc.FANOUT, active_set_size=dc.ASZ, rotation_probability=0.0, seed=dc.SEED,
                    bfs_mode=bfs, profile=True)
    for u, outs in edges.items():
        for k in range(25):
            eng.set_entry(ids[u], k, [ids[v] for v in outs])
    ex = drive(eng, stakes, [ids["o"]], 1, init=False, tag="cascade")
    idom, parent = reference(eng, 0, ids["o"])[0], eng.tree(0).tolist()
    for z, p in (("c6", "c5"), ("c5", "c4"), ("c4", "c3"), ("c3", "c2")):
        assert parent[ids[z]] == ids[p] and idom[ids[z]] == ids["o"], z
    assert idom[ids["c7"]] == ids["c6"] and idom[ids["a5"]] == ids["c5"] and ex.moved == 4
    assert eng.kernel_time("tree_stake")[1] > launches_per_round(1)  # more than one sweep ran
    eng.close()


@gpu
@pytest.mark.parametrize("bfs", MODES)
def test_chain_253_levels_one_launch_per_sweep(bfs):
    case, rounds = dc.chain_case(253), 2
    eng = dc.chain_engine(case, 2, bfs_mode=bfs, profile=True)
    ex = drive(eng, case["stakes"], case["c"][:2], rounds, init=False, tag="chain")
    assert ex.moved == 0 and ex.same >= 253 and ex.last[0]["subtree"][case["c"][0]] >= 253
    assert eng.kernel_time("tree_stake")[1] == launches_per_round(1) * rounds  # the thin run is one launch
    eng.close()


@gpu
def test_lifecycle(monkeypatch):
    n, s, E = tv.N1, tv.S1, ts.GS_ESTATE
    eng, off = tv.engine1(monkeypatch, "level"), tv.engine1(monkeypatch, "level")
    for e in (eng, off):
        e.set_slots(tv.ORIGINS1)
        e.init_active_sets()
    dominators = lambda: eng.enable_tree_stake(records=True, dominators=True)
    raises(E, dominators, "gs_tree_enable_records")  # no records tree
    for e in (eng, off):
        e.enable_tree(records=True)
    b0 = ts.sizes(eng)
    raises(E, lambda: eng.dominators(0))  # the kind is not on
    dominators()
    dominators()  # twice: a no-op
    assert ts.sizes(eng)["pair_bytes"] - b0["pair_bytes"] == 20 * s * n
    raises(E, lambda: eng.enable_tree_stake(records=True))  # each kind refuses while another is on
    raises(E, eng.enable_tree_stake)
    raises(E, lambda: eng.dominators(0))  # no round recorded yet
    for e in (eng, off):
        e.round(0, record=True)
    raises(ts.GS_EINVAL, lambda: eng.dominators(s))
    assert eng.dominators(0)[tv.ORIGINS1[0]] == NONE
    for j in range(s):  # the first-delivery arrays do not see the kind
        assert np.array_equal(eng.tree(j), off.tree(j))
        assert all(np.array_equal(a, b) for a, b in zip(eng.tree_load(j), off.tree_load(j)))
    eng.set_slots(tv.ORIGINS1)  # zeroes the view
    raises(E, lambda: eng.dominators(0))
    eng.enable_tree_stake(False)
    assert ts.sizes(eng) == b0
    eng.enable_tree_stake(records=True)
    raises(E, dominators)
    eng.enable_tree_stake(False)
    dominators()
    eng.enable_tree(False)  # turning the tree off frees the kind as well
    raises(E, lambda: eng.dominators(0))
    for e in (eng, off):
        e.close()
