"""The delivery tree in stake (gs_tree_stake_enable[_groups]), exactly equal to an
expectation built in Python ints from Engine.tree(slot), Engine.hops(slot) and the stakes after each
recorded round (bottom-up in descending hop order), the grouping and the weights. Engine.tree is
pinned to the oracle by test_tree.py / test_tree_records.py."""
import numpy as np
import pytest

import degenerate_case as dc
import test_cluster_view as tv
from test_cluster_groups import raises

gs, synth = tv.gs, tv.synth
pytestmark = pytest.mark.gpu

GS_EINVAL, GS_ERANGE, GS_ESTATE = -1, -4, -5
NONE, UP_THREADS = 0xFFFFFFFF, 512  # k_tstake_up's workgroup: a level above it takes several trips
KEYS = ("children", "subtree", "below")
# the one-kernel round with enable_tree(), the step-wise round with the records mode
MODES = {"wg": (gs.GS_BFS_WORKGROUP, False), "level": (gs.GS_BFS_LEVEL, True)}


class Expect:
    def __init__(self, stakes, groups, weights):
        self.st, self.groups, self.w = [int(x) for x in stakes], list(groups), [int(x) for x in weights]
        n = len(self.st)
        self.tot = [{k: [0] * n for k in KEYS} for _ in self.groups]
        self.last, self.rounds, self.widest, self.below_max, self.unreached = None, 0, 0, 0, 0

    def record(self, eng, what=""):
        n, self.last, j0 = len(self.st), [], 0
        for g, ns in enumerate(self.groups):
            last = {k: [0] * n for k in KEYS}
            for j in range(j0, j0 + ns):
                parent, hops = eng.tree(j).tolist(), eng.hops(j).tolist()
                kids, sub, below = [0] * n, [0] * n, [0] * n
                for w in sorted((w for w in range(n) if parent[w] != NONE), key=lambda w: -hops[w]):
                    p = parent[w]
                    kids[p], sub[p], below[p] = kids[p] + 1, sub[p] + sub[w] + 1, below[p] + below[w] + self.st[w]
                assert [int(x) for x in eng.tree_stake(j)] == below, f"{what}: slot {j} below"
                self.widest = max(self.widest, np.bincount([h for h in hops if 0 < h < 255] or [0]).max())
                self.below_max = max(self.below_max, max(below))
                self.unreached += hops.count(255)
                for k, a in zip(KEYS, (kids, sub, below)):
                    last[k] = [x + self.w[j] * y for x, y in zip(last[k], a)]
            j0 += ns
            for k in KEYS:
                self.tot[g][k] = [x + y for x, y in zip(self.tot[g][k], last[k])]
            self.last.append(last)
        self.rounds += 1

    def check(self, eng, what=""):
        for g in range(len(self.groups)):
            r = eng.tree_stake_load(g)
            assert r["rounds"] == self.rounds and r["children"].dtype == r["last_subtree"].dtype == np.uint64, what
            for k in KEYS:
                assert [int(x) for x in r[k]] == self.tot[g][k], f"{what}: group {g} {k}"
                assert [int(x) for x in r["last_" + k]] == self.last[g][k], f"{what}: group {g} last_{k}"


def engine(mode, st, s, **kw):
    bfs, _ = MODES[mode]
    return gs.Engine(st, s, bfs_mode=bfs, **{**dict(seed=23, active_set_size=12, rotation_probability=0.1), **kw})


def drive(eng, mode, st, origins, rounds, groups=None, weights=None, *, fractions=None, init=True, tag=""):
    s = len(origins)
    ex = Expect(st, groups if isinstance(groups, list) else [s], weights or [1] * s)
    eng.set_slots(origins, 2, 0.15)
    if init:
        eng.init_active_sets()
    eng.enable_tree(records=MODES[mode][1])
    eng.enable_tree_stake(groups=groups, weights=weights)
    if fractions:
        eng.fail_nodes(fractions)
    for r in range(rounds):
        eng.round(r, record=True)
        ex.record(eng, f"{tag} round {r}")
        ex.check(eng, f"{tag} round {r}")
    return ex


def by_stake_rank(st, ranks):
    top = sorted((int(x) for x in st), reverse=True)
    return [int(np.nonzero(st == np.uint64(top[r - 1]))[0][0]) for r in ranks]


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", ["tiny7", "groups131", "trips1050", "wide131"])
def test_tree_stake_matches_python(case, mode):
    if case == "tiny7":  # fewer nodes than a wave
        st = synth.network(7)[1]
        eng = engine(mode, st, 2)
        ex = drive(eng, mode, st, [1, 5], 6, tag=case)
    elif case == "groups131":  # the chunk table, a skipped slot, unreached nodes
        st = synth.network(tv.N1)[1]
        eng = engine(mode, st, tv.S1)
        ex = drive(eng, mode, st, tv.ORIGINS1, 8, [3, 1, 3], [1, 2, 0, 5, 1, 1, 3], fractions=[0.3] * tv.S1, tag=case)
        assert ex.unreached > 0, "every node was reached"
    elif case == "trips1050":  # test_tree.py's shape: a level wider than the workgroup
        st = synth.network(1050)[1]
        eng = engine(mode, st, 4, seed=11, fanout=6)
        ex = drive(eng, mode, st, by_stake_rank(st, (1, 131, 525, 1049)), 3, tag=case)
        assert ex.widest > UP_THREADS, "no level wider than k_tstake_up's workgroup"
    else:  # stakes near 2^64 / (2 N): below uses most of u64, round values pass 2^64, totals carry
        n = tv.N1
        st = np.array([2**64 // (2 * n) - 977 * v for v in range(n)], dtype=np.uint64)
        assert sum(int(x) for x in st) < 2**64 and tv.S1 * 40_000 * n < 2**32
        eng = engine(mode, st, tv.S1)
        ex = drive(eng, mode, st, tv.ORIGINS1, 4, [3, 1, 3], [40_000] * tv.S1, tag=case)
        assert ex.below_max >= 2**62 and max(ex.last[0]["below"]) >= 2**64 and max(ex.tot[0]["below"]) >= 2**65
    assert ex.rounds > 0 and sum(ex.tot[0]["subtree"]) > 0
    eng.close()


@pytest.mark.parametrize("mode", list(MODES))
def test_chain_253_levels(mode):
    case = dc.chain_case(253)
    eng = dc.chain_engine(case, 2, bfs_mode=MODES[mode][0])
    ex = drive(eng, mode, case["stakes"], case["c"][:2], 3, init=False, tag="chain")
    head = case["c"][0]  # from the chain's head every subtree is a suffix of the chain
    assert ex.last[0]["subtree"][head] >= 253 and ex.last[0]["below"][head] >= 253 * dc.STAKE and ex.widest <= 2
    eng.close()


@pytest.mark.parametrize("multi", [False, True])
def test_one_group_per_table(multi):
    st = synth.network(tv.N1)[1]
    kw = dict(bfs_mode=gs.GS_BFS_MULTI, traj_multi=True) if multi else dict(bfs_mode=gs.GS_BFS_WORKGROUP)
    eng = gs.Engine(st, tv.S1, seed=23, trajectories=[(4, 0.1, 3), (12, 0.0, 4)], **kw)
    ex = Expect(st, [3, 4], [1] * tv.S1)
    eng.set_slots(tv.ORIGINS1)
    eng.init_active_sets()
    eng.enable_tree(records=multi)
    eng.enable_tree_stake(groups="tables")
    for r in range(5):
        eng.round(r, record=r >= 1)
        if r >= 1:
            ex.record(eng, f"tables round {r}")
    ex.check(eng, "tables")
    eng.close()


def raw_enable(eng, groups, n_groups):
    g = None if groups is None else np.ascontiguousarray(groups, dtype=np.uint32)
    gs._check(gs.lib().gs_tree_stake_enable_groups(eng.h, None if g is None else gs._ptr(g), n_groups, None))


def sizes(eng):
    return {k: eng.info()[k] for k in ("device_bytes", "pair_bytes", "other_bytes")}


def test_lifecycle(monkeypatch):
    st = synth.network(tv.N1)[1]
    n, s = tv.N1, tv.S1
    eng, off = tv.engine1(monkeypatch, "wg_fused", profile=True), tv.engine1(monkeypatch, "wg_fused", profile=True)
    for e in (eng, off):
        e.set_slots(tv.ORIGINS1)
        e.init_active_sets()
    raises(GS_ESTATE, eng.tree_stake_load)
    raises(GS_ESTATE, eng.enable_tree_stake, "gs_tree_enable")  # no tree mode
    eng.enable_tree()
    b0 = sizes(eng)
    for bad, ng, word in (([3, 1, 2], 3, "group_slots"), ([3, 0, 4], 3, "group_slots[1]"), ([1] * 8, 8, "n_groups"),
                          (None, 3, "group_slots")):
        raises(GS_EINVAL, lambda: raw_enable(eng, bad, ng), word)
    raises(GS_ERANGE, lambda: eng.enable_tree_stake(weights=[2**23] * s), "group 0")  # 7 x 2^23 x 131 >= 2^32
    assert sizes(eng) == b0
    groups, weights = [3, 1, 3], [1, 2, 0, 5, 1, 1, 3]
    eng.enable_tree_stake(groups=groups, weights=weights)
    eng.enable_tree_stake(groups=groups, weights=weights)  # twice: a no-op
    raises(GS_ESTATE, lambda: eng.enable_tree_stake(groups=[3, 2, 2], weights=weights))
    raises(GS_ESTATE, eng.enable_tree_stake)
    raises(GS_ESTATE, lambda: eng.tree_stake(0))  # no round recorded yet
    raises(GS_ESTATE, lambda: eng.tree_stake_load(0))
    b1 = sizes(eng)
    assert b1["pair_bytes"] - b0["pair_bytes"] == 12 * s * n
    assert b1["other_bytes"] - b0["other_bytes"] >= 3 * n * 96 + 4 * s
    ex = Expect(st, groups, weights)
    for e in (eng, off):
        e.kernel_time_reset()
        for r in range(8):
            e.round(r, record=r % 2 == 1)
            if e is eng and r % 2 == 1:
                ex.record(eng, f"round {r}")
    ex.check(eng, "every other round recorded")
    assert eng.kernel_time("tree_stake")[1] == 3 * 4 and off.kernel_time("tree_stake")[1] == 0
    raises(GS_EINVAL, lambda: eng.tree_stake_load(3))
    raises(GS_EINVAL, lambda: eng.tree_stake(s))
    eng.set_slots(tv.ORIGINS1)  # zeroes the view and its round count
    raises(GS_ESTATE, lambda: eng.tree_stake_load(1))
    eng.round(8, record=True)
    off.set_slots(tv.ORIGINS1)
    off.round(8, record=True)
    r = eng.tree_stake_load(1)
    assert r["rounds"] == 1 and list(r["below"]) == list(r["last_below"]) and any(r["below"])
    eng.enable_tree_stake(False)
    assert sizes(eng) == b0
    eng.enable_tree_stake()
    eng.enable_tree(False)  # turning the tree off frees the view as well
    raises(GS_ESTATE, lambda: eng.tree_stake(0))
    assert eng.info()["device_bytes"] == b0["device_bytes"] - 12 * s * n
    for e in (eng, off):  # the engine whose view is off again equals the twin that never had one
        e.round(9, record=True)
    assert eng.summaries().tobytes() == off.summaries().tobytes()
    for j in range(s):
        assert np.array_equal(eng.hops(j), off.hops(j))
        for u, v in zip(eng.caches(j), off.caches(j)):
            assert np.array_equal(u, v), f"caches of slot {j}"
    for e in (eng, off):
        e.close()
    heavy = gs.Engine(np.array([2**63, 2**63, 1], dtype=np.uint64), 1, seed=5, bfs_mode=gs.GS_BFS_WORKGROUP)
    heavy.enable_tree()
    raises(GS_ERANGE, heavy.enable_tree_stake, "2^64")
    heavy.close()
    big = gs.Engine(synth.network(10_200)[1], 1, seed=5, bfs_mode=gs.GS_BFS_LEVEL)  # past the LDS bound of 10,175
    big.enable_tree(records=True)
    raises(GS_ERANGE, big.enable_tree_stake, "10175 nodes")
    big.close()
    part = gs.Engine(st, s, seed=23, active_set_size=12, rotation_probability=0.1, part=(0, 1))
    raises(GS_ESTATE, part.enable_tree_stake)
    part.close()
