"""The stake reach view (gs_reach_enable[_groups]), exactly equal to an expectation built in Python
ints from Engine.hops(slot) after each recorded round, the stakes, the grouping and the weights."""
import numpy as np
import pytest

import degenerate_case as dc
import test_cluster_view as tv
from test_cluster_groups import raises

gs, synth = tv.gs, tv.synth
pytestmark = pytest.mark.gpu

GS_EINVAL, GS_ERANGE, GS_ESTATE = -1, -4, -5
GROUPS1, WEIGHTS1 = [3, 1, 3], [1, 2, 0, 5, 1, 1, 3]


class Expect:
    def __init__(self, stakes, groups, weights):
        self.st = [int(x) for x in stakes]
        self.groups, self.w = list(groups), [int(x) for x in weights]
        G = len(self.groups)
        self.nodes, self.stake = [[0] * 256 for _ in range(G)], [[0] * 256 for _ in range(G)]
        self.last_nodes, self.last_stake, self.rounds, self.widest, self.carried = None, None, 0, 0, False

    def record(self, eng):
        self.last_nodes, self.last_stake, j = [], [], 0
        for g, ns in enumerate(self.groups):
            ln, ls = [0] * 256, [0] * 256
            for j in range(j, j + ns):
                for v, b in enumerate(eng.hops(j).tolist()):
                    ln[b] += self.w[j]
                    ls[b] += self.w[j] * self.st[v]
            j += 1
            for b in range(256):
                self.carried |= (self.stake[g][b] % 2**64) + (ls[b] % 2**64) >= 2**64
                self.nodes[g][b] += ln[b]
                self.stake[g][b] += ls[b]
            self.widest = max(self.widest, max(ls))
            self.last_nodes, self.last_stake = self.last_nodes + [ln], self.last_stake + [ls]
        self.rounds += 1

    def check(self, eng, what=""):
        for g in range(len(self.groups)):
            r = eng.reach(g)
            assert r["nodes"].dtype == r["last_nodes"].dtype == np.uint64 and r["rounds"] == self.rounds, what
            for k in ("nodes", "stake", "last_nodes", "last_stake"):
                assert [int(x) for x in r[k]] == getattr(self, k)[g], f"{what}: group {g} {k}"


def drive(eng, stakes, origins, rounds, groups=None, weights=None, *, first=0, fail_at=None, every=4, tag=""):
    s = len(origins)
    ex = Expect(stakes, groups or [s], weights or [1] * s)
    eng.set_slots(origins)
    eng.enable_reach(groups=groups, weights=weights)
    eng.init_active_sets()
    for r in range(rounds):
        if r == fail_at:
            eng.fail_nodes(tv.FRACTIONS1)
        eng.round(r, record=r >= first)
        if r >= first:
            ex.record(eng)
            if (r - first) % every == 0 or r == rounds - 1:
                ex.check(eng, f"{tag} round {r}")
    return ex


# (the last case: a round's stake passes 2^64 and the totals carry; 7 x 40,000 x 131 < 2^32)
@pytest.mark.parametrize("path,weights", [(p, WEIGHTS1) for p in tv.PATHS] + [("wg_fused", [40_000] * tv.S1)])
def test_every_round_path(monkeypatch, path, weights):
    eng = tv.engine1(monkeypatch, path)
    st = synth.network(tv.N1)[1]
    ex = drive(eng, st, tv.ORIGINS1, tv.ROUNDS1, GROUPS1, weights, first=2, fail_at=3, every=6, tag=path)
    assert ex.rounds == tv.ROUNDS1 - 2 and not eng.info()["round_split"]
    assert any(s[255] > 0 for s in ex.stake), "no unreached stake: bin 255 was idle"
    assert all(sum(x > 0 for x in s) > 2 for s in ex.stake)
    if weights is not WEIGHTS1:
        assert ex.widest >= 2**64, "no single-round stake value needs the high half"
        assert ex.carried, "no total carried out of its low half"
    eng.close()


@pytest.mark.parametrize("mode,n,s,per_slot", [("wg", 67, 70, False), ("wg", 67, 70, True), ("level", 67, 70, False),
                                               ("level", 67, 70, True), ("wg", 3, 3, False),
                                               ("level", 1025, 5, False), ("multi", 1025, 5, False)])
def test_node_block_and_chunk_edges(mode, n, s, per_slot):
    _, st = synth.network(n)
    bfs = {"wg": gs.GS_BFS_WORKGROUP, "level": gs.GS_BFS_LEVEL, "multi": gs.GS_BFS_MULTI}[mode]
    eng = gs.Engine(st, s, seed=5, active_set_size=12, rotation_probability=0.1, bfs_mode=bfs)
    ex = drive(eng, st, [j % n for j in range(s)], 8, [1] * s if per_slot else None, tag=f"{mode} n={n} s={s}")
    assert ex.rounds == 8 and sum(ex.nodes[0]) == 8 * n * (1 if per_slot else s)
    eng.close()


@pytest.mark.parametrize("mode", [gs.GS_BFS_LEVEL, gs.GS_BFS_WORKGROUP])
def test_deep_hops(mode):
    case = dc.chain_case(253)
    eng = dc.chain_engine(case, 2, bfs_mode=mode)
    eng.set_slots(case["c"][:2], 2, 0.15)
    eng.enable_reach()
    ex = Expect(case["stakes"], [2], [1, 1])
    for r in range(3):
        eng.round(r, record=True)
        ex.record(eng)
        ex.check(eng, f"chain round {r}")
    assert all(ex.stake[0][b] >= dc.STAKE for b in range(254)), "a hop bin of the chain is empty"
    assert ex.last_nodes[0][255] >= 2 * case["spare"] and ex.stake[0][254] == 0
    eng.close()


def raw_enable(eng, groups, n_groups):
    g = None if groups is None else np.ascontiguousarray(groups, dtype=np.uint32)
    gs._check(gs.lib().gs_reach_enable_groups(eng.h, None if g is None else gs._ptr(g), n_groups, None))


def test_lifecycle(monkeypatch):
    st = synth.network(tv.N1)[1]
    eng, off = tv.engine1(monkeypatch, "wg_fused", profile=True), tv.engine1(monkeypatch, "wg_fused", profile=True)
    b0 = eng.info()
    raises(GS_ESTATE, eng.reach)
    for bad, n, word in (([3, 1, 2], 3, "group_slots"), ([3, 0, 4], 3, "group_slots[1]"), ([1] * 8, 8, "n_groups"),
                         (None, 3, "group_slots")):
        raises(GS_EINVAL, lambda: raw_enable(eng, bad, n), word)
    assert eng.info()["device_bytes"] == b0["device_bytes"]
    for e in (eng, off):
        e.set_slots(tv.ORIGINS1)
    eng.enable_reach(groups=GROUPS1, weights=WEIGHTS1)
    eng.enable_reach(groups=GROUPS1, weights=WEIGHTS1)  # twice: a no-op
    raises(GS_ESTATE, lambda: eng.enable_reach(groups=[3, 2, 2], weights=WEIGHTS1))
    raises(GS_ESTATE, eng.enable_reach)
    raises(GS_EINVAL, lambda: eng.reach(3))
    b1 = eng.info()
    assert b1["device_bytes"] - b0["device_bytes"] >= 3 * 18 * 1024 and b1["pair_bytes"] == b0["pair_bytes"]
    assert b1["other_bytes"] - b0["other_bytes"] == b1["device_bytes"] - b0["device_bytes"]
    eng.enable_cluster_view()  # both views at once, with different groupings
    cl = tv.Expect(tv.N1)
    ex = Expect(st, GROUPS1, WEIGHTS1)
    for e in (eng, off):
        e.init_active_sets()
        e.kernel_time_reset()
        for r in range(10):
            e.round(r, record=r % 2 == 1)
            if e is eng and r % 2 == 1:
                ex.record(eng)
                cl.record(eng)
    ex.check(eng, "with the cluster view")
    cl.check(eng, "beside the reach view")
    assert eng.kernel_time("reach")[1] == 2 * 5 and off.kernel_time("reach")[1] == 0
    assert eng.summaries().tobytes() == off.summaries().tobytes()
    for j in range(tv.S1):
        assert np.array_equal(eng.hops(j), off.hops(j))
        for u, v in zip(eng.accumulators(j), off.accumulators(j)):
            assert np.array_equal(u, v), f"accumulators of slot {j}"
    eng.set_slots(tv.ORIGINS1)  # zeroes the view and its round count
    r = eng.reach(1)
    assert r["rounds"] == 0 and not r["nodes"].any() and not any(r["stake"]) and not any(r["last_stake"])
    eng.enable_cluster_view(False)
    eng.enable_reach(False)
    assert eng.info()["device_bytes"] == b0["device_bytes"]
    raises(GS_ESTATE, eng.reach)
    for e in (eng, off):
        e.close()
    tiny = gs.Engine(synth.network(3)[1], 1, seed=5, active_set_size=12, bfs_mode=gs.GS_BFS_WORKGROUP)
    raises(GS_ERANGE, lambda: tiny.enable_reach(weights=[2**31]), "group 0")  # 3 nodes x 2^31 >= 2^32
    raises(GS_ESTATE, tiny.reach)
    tiny.close()
    part = gs.Engine(st, tv.S1, seed=23, active_set_size=12, rotation_probability=0.1, part=(0, 1))
    raises(GS_ESTATE, part.enable_reach)
    part.close()
