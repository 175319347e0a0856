"""The cluster load view per slot group, with a weight per slot (gs_cluster_enable_groups).

As in test_cluster_view.py the expectation is built in numpy from the per-slot readbacks, which
the parity tests pin to the oracle: after each recorded round, Engine.counters(slot) (egress of an
unreached node already reads 0) and Engine.hops(slot) of the slots of a group are summed, each
times its slot's weight, into that group's E, I, P, D, H; totals, peaks and the gs_cluster_round
struct (np.argmax: the smallest id among equal maxima) accumulate from them per group. Every
comparison is exact equality.
"""
import ctypes as C

import numpy as np
import pytest

import engine_bind as eb
import test_cluster_view as tv

gs = eb.gs
synth = eb.synth
pytestmark = pytest.mark.gpu

GS_EINVAL, GS_ERANGE, GS_ESTATE = -1, -4, -5
TOTALS = tv.TOTALS
PEAKS = ("egress_peak", "ingress_peak")


class GExpect:
    """The grouped view's definition, restated over the per-slot readbacks."""

    def __init__(self, n, groups, weights):
        self.n, self.groups, self.weights = n, list(groups), [int(w) for w in weights]
        G = len(self.groups)
        self.tot = [{k: np.zeros(n, dtype=np.uint64) for k in TOTALS} for _ in range(G)]
        self.peak = [{k: np.zeros(n, dtype=np.uint32) for k in PEAKS} for _ in range(G)]
        self.rounds = [[] for _ in range(G)]
        self.unreached = 0  # (slot, node) pairs unreached in a recorded round

    def record(self, eng):
        start = 0
        for g, ng in enumerate(self.groups):
            r = {k: np.zeros(self.n, dtype=np.uint64) for k in TOTALS}
            for j in range(start, start + ng):
                w = np.uint64(self.weights[j])
                e, i, p = eng.counters(j)
                h = eng.hops(j).astype(np.uint64)
                d = ((h >= 1) & (h <= 254)).astype(np.uint64)
                self.unreached += int((h == 0xFF).sum())
                r["egress"] += w * e.astype(np.uint64)
                r["ingress"] += w * i.astype(np.uint64)
                r["prunes"] += w * p.astype(np.uint64)
                r["delivered"] += w * d
                r["hop_sum"] += w * h * d
            start += ng
            assert all(int(r[k].max()) < 2**32 for k in TOTALS)  # (the enable rule keeps a round's sums in u32)
            for k in TOTALS:
                self.tot[g][k] += r[k]
            self.peak[g]["egress_peak"] = np.maximum(self.peak[g]["egress_peak"], r["egress"].astype(np.uint32))
            self.peak[g]["ingress_peak"] = np.maximum(self.peak[g]["ingress_peak"], r["ingress"].astype(np.uint32))
            self.rounds[g].append(dict(
                pushes=int(r["egress"].sum()), ingress=int(r["ingress"].sum()), prunes=int(r["prunes"].sum()),
                delivered=int(r["delivered"].sum()), egress_max=int(r["egress"].max()),
                egress_max_node=int(np.argmax(r["egress"])), ingress_max=int(r["ingress"].max()),
                ingress_max_node=int(np.argmax(r["ingress"])), senders=int((r["egress"] > 0).sum()), pad0=0))

    def check(self, eng, what=""):
        n_sum = len(eng.summaries())
        for g in range(len(self.groups)):
            got = eng.cluster_load(g)
            for k in TOTALS:
                assert got[k].dtype == np.uint64 and np.array_equal(got[k], self.tot[g][k]), f"{what}: group {g} total {k}"
            for k, v in self.peak[g].items():
                assert got[k].dtype == np.uint32 and np.array_equal(got[k], v), f"{what}: group {g} {k}"
            cr = eng.cluster_rounds(g)
            assert len(cr) == len(self.rounds[g]) == n_sum, f"{what}: group {g}: {len(cr)} cluster rounds"
            for r, exp in enumerate(self.rounds[g]):
                for k, v in exp.items():
                    assert int(cr[r][k]) == v, f"{what}: group {g} round {r} {k}: {int(cr[r][k])} != {v}"


def drive(eng, origins, rounds, groups, weights, *, first_recorded=0, fail_at=None, fractions=None, every=1, tag=""):
    """set_slots, the grouped view on, init, `rounds` rounds (recorded from first_recorded on); the
    expectation is updated after every recorded round and compared every `every` of them."""
    eng.set_slots(origins)
    eng.enable_cluster_view(groups=groups, weights=weights)
    gsz, w = eng.cluster_groups()
    ex = GExpect(eng.n, gsz.tolist(), w.tolist())
    eng.init_active_sets()
    for r in range(rounds):
        if fail_at is not None and r == fail_at:
            eng.fail_nodes(fractions)
        rec = r >= first_recorded
        eng.round(r, record=rec)
        if rec:
            ex.record(eng)
            if (r - first_recorded) % every == 0 or r == rounds - 1:
                ex.check(eng, f"{tag} round {r}")
    return ex


def same_group(a, ga, b, gb, what=""):
    """group ga of engine a and group gb of engine b hold the same view (None: the un-suffixed reads)"""
    la, lb = a.cluster_load(ga), b.cluster_load(gb)
    for k in TOTALS + PEAKS:
        assert la[k].dtype == lb[k].dtype and np.array_equal(la[k], lb[k]), f"{what}: {k}"
    ra, rb = a.cluster_rounds(ga), b.cluster_rounds(gb)
    assert len(ra) == len(rb) > 0 and ra.tobytes() == rb.tobytes(), f"{what}: rounds"


# --- 1. every round path -----------------------------------------------------------------
N1, S1, ROUNDS1, ORIGINS1, FRACTIONS1 = tv.N1, tv.S1, tv.ROUNDS1, tv.ORIGINS1, tv.FRACTIONS1
GROUPS1, WEIGHTS1 = [3, 1, 3], [1, 2, 0, 5, 1, 1, 3]
assert (N1, S1, ROUNDS1) == (131, 7, 26) and FRACTIONS1 == [0.0, 0.3, 0.0, 0.0, 0.3, 0.0, 0.0]


@pytest.mark.parametrize("path", list(tv.PATHS))
def test_every_round_path(monkeypatch, path):
    """Groups (3, 1, 3): on the node-major egress of multi / hybrid (SP = 8) group 1 is the single
    slot 3, the last byte of a word, group 2 starts on slot 4 and its last word holds one pad byte;
    the zero-weight slot 2 closes group 0."""
    eng = tv.engine1(monkeypatch, path)
    if path.startswith("wg_fused"):
        assert eng.info()["fused_round"]
    ex = drive(eng, ORIGINS1, ROUNDS1, GROUPS1, WEIGHTS1, first_recorded=2, fail_at=3, fractions=FRACTIONS1, tag=path)
    assert ex.groups == GROUPS1 and ex.weights == WEIGHTS1
    assert all(len(r) == ROUNDS1 - 2 for r in ex.rounds)  # rounds 0 and 1 do not count
    assert sum(int(t["prunes"].sum()) for t in ex.tot) > 0, "no prune wave within the case's rounds"
    assert ex.unreached > 0, "every (slot, node) was reached in every recorded round: no stale egress byte"
    assert not eng.info()["round_split"]  # (off while any view is on)
    eng.close()


# --- 2. slot-split, group-boundary and node-block edges ------------------------------------------
MODES = {"wg": gs.GS_BFS_WORKGROUP, "level": gs.GS_BFS_LEVEL, "multi": gs.GS_BFS_MULTI}
EDGES = [(m, n, s, g) for m in MODES for n, s, g in [
    (67, 70, (1, 64, 5)),         # wave splits inside a group; boundaries at slots 1 and 65
    (67, 70, (17, 17, 17, 19)),   # boundaries at 17, 34, 51: every residue mod 4
    (3, 3, (1, 1, 1)),            # ties on the max node
    (1025, 5, (2, 3)),            # two node blocks of the fold, five of the reduction
    (67, 1, (1,)),                # S = 1, G = 1, weight 7
]]


@pytest.mark.parametrize("mode,n,s,groups", EDGES)
def test_group_edges(mode, n, s, groups):
    _, st = synth.network(n)
    eng = gs.Engine(st, s, seed=5, active_set_size=12, rotation_probability=0.1, bfs_mode=MODES[mode])
    weights = [7] if s == 1 else [(3 * j + 1) % 5 for j in range(s)]  # (zeros among them)
    ex = drive(eng, [j % n for j in range(s)], 8, list(groups), weights, every=4, tag=f"{mode} n={n} s={s} {groups}")
    assert all(len(r) == 8 for r in ex.rounds) and sum(int(t["egress"].sum()) for t in ex.tot) > 0
    eng.close()


# --- 3. table engines: a group per table equals the table's own engine ------------------------
@pytest.mark.parametrize("seeded", [False, True])
@pytest.mark.parametrize("multi", [False, True])
def test_tables(seeded, multi):
    _, st = synth.network(N1)
    tables, seeds = [(4, 0.1, 3), (12, 0.0, 4)], (7, 8) if seeded else (23, 23)
    if seeded:
        tables = [t + (sd,) for t, sd in zip(tables, seeds)]
    mode = dict(bfs_mode=gs.GS_BFS_MULTI) if multi else {}
    eng = gs.Engine(st, S1, seed=23, trajectories=tables, **(dict(traj_multi=True, **mode) if multi else {}))
    ex = drive(eng, ORIGINS1, 10, "tables", None, first_recorded=1, every=3, tag=f"tables seeded={seeded} multi={multi}")
    gsz, w = eng.cluster_groups()
    assert gsz.tolist() == [3, 4] and w.tolist() == [1] * S1
    assert sum(int(t["delivered"].sum()) for t in ex.tot) > 0
    s0 = 0
    for g, (asz, p, ns) in enumerate(t[:3] for t in tables):  # the table alone: its slots, origins and seed
        one = gs.Engine(st, ns, seed=seeds[g], active_set_size=asz, rotation_probability=p, **mode)
        one.set_slots(ORIGINS1[s0:s0 + ns])
        one.enable_cluster_view()
        one.init_active_sets()
        for r in range(10):
            one.round(r, record=r >= 1)
        same_group(eng, g, one, None, f"table {g} seeded={seeded} multi={multi}")
        one.close()
        s0 += ns
    eng.close()


# --- 4. consistency with the ungrouped view ---------------------------------------------------
def run1(eng, enable):
    eng.set_slots(ORIGINS1)
    enable(eng)
    eng.init_active_sets()
    for r in range(ROUNDS1):
        if r == 3:
            eng.fail_nodes(FRACTIONS1)
        eng.round(r, record=r >= 2)
    return eng


@pytest.mark.parametrize("path", ["wg_fused", "multi"])
def test_consistent_with_the_ungrouped_view(monkeypatch, path):
    plain = run1(tv.engine1(monkeypatch, path), lambda e: e.enable_cluster_view())
    one = run1(tv.engine1(monkeypatch, path), lambda e: e.enable_cluster_view(groups=[S1]))
    three = run1(tv.engine1(monkeypatch, path), lambda e: e.enable_cluster_view(groups=GROUPS1))
    same_group(one, None, plain, None, "G = 1, unit weights")  # every array and every round struct
    same_group(one, 0, plain, 0, "G = 1 through the _group reads")
    load, cr = plain.cluster_load(), plain.cluster_rounds()
    parts = [(three.cluster_load(g), three.cluster_rounds(g)) for g in range(3)]
    for k in TOTALS:  # with unit weights the groups' totals add up to the ungrouped view's
        assert np.array_equal(sum(p[0][k] for p in parts), load[k]), k
    for k in ("pushes", "ingress", "prunes", "delivered"):
        assert np.array_equal(sum(p[1][k] for p in parts), cr[k]), k
    for k in PEAKS:  # peaks and maxima are bounded by it (a group's peak round need not be the view's)
        assert all((p[0][k] <= load[k]).all() for p in parts) and (sum(p[0][k].astype(np.uint64) for p in parts) >= load[k]).all()
    for k in ("egress_max", "ingress_max", "senders"):
        assert all((p[1][k] <= cr[k]).all() for p in parts), k
    assert load["prunes"].sum() > 0
    for e in (plain, one, three):
        e.close()


# --- 5. the view changes nothing ---------------------------------------------------------------
@pytest.mark.parametrize("path", ["wg_fused", "multi"])
def test_view_changes_nothing(monkeypatch, path):
    on = run1(tv.engine1(monkeypatch, path), lambda e: e.enable_cluster_view(groups=GROUPS1, weights=WEIGHTS1))
    off = run1(tv.engine1(monkeypatch, path), lambda e: None)
    a, b = on.summaries(), off.summaries()
    assert a.shape == b.shape == (ROUNDS1 - 2, S1) and a.tobytes() == b.tobytes()
    for j in range(S1):
        for u, v in zip(on.accumulators(j), off.accumulators(j)):
            assert np.array_equal(u, v), f"accumulators of slot {j}"
        for u, v in zip(on.caches(j), off.caches(j)):
            assert np.array_equal(u, v), f"caches of slot {j}"
    assert sum(int(on.cluster_load(g)["prunes"].sum()) for g in range(3)) > 0
    on.close()
    off.close()


# --- 6. bounds and lifecycle --------------------------------------------------------------------
def raises(code, fn, *words):
    with pytest.raises(gs.GsError) as ei:
        fn()
    assert ei.value.code == code, str(ei.value)
    for w in words:
        assert w in str(ei.value), str(ei.value)


def engine6(s=S1, **kw):
    _, st = synth.network(N1)
    return gs.Engine(st, s, seed=23, active_set_size=12, rotation_probability=0.1, bfs_mode=gs.GS_BFS_WORKGROUP, **kw)


def test_weight_bound():
    wmax = (2**32 - 1) // 255  # max(255, inbound capacity): the default capacity is 64
    engs = []
    for weights in ([wmax, 1], [1, 1]):
        eng = engine6(2)
        eng.set_slots([0, 77])
        eng.enable_cluster_view(groups=[1, 1], weights=weights)
        eng.init_active_sets()
        for r in range(6):
            eng.round(r, record=True)
        engs.append(eng)
    big, unit = engs
    lb, lu = big.cluster_load(0), unit.cluster_load(0)
    assert lu["egress"].sum() > 0 and lu["egress_peak"].max() > 0
    for k in TOTALS + PEAKS:  # w x the unit-weight results, no wrap
        assert np.array_equal(lb[k].astype(np.uint64), lu[k].astype(np.uint64) * np.uint64(wmax)), k
    rb, ru = big.cluster_rounds(0), unit.cluster_rounds(0)
    for k in ("pushes", "ingress", "prunes", "delivered", "egress_max", "ingress_max"):
        assert np.array_equal(rb[k].astype(np.uint64), ru[k].astype(np.uint64) * np.uint64(wmax)), k
    for k in ("egress_max_node", "ingress_max_node", "senders"):
        assert np.array_equal(rb[k], ru[k]), k
    same_group(big, 1, unit, 1, "the unit-weight group beside it")
    for e in engs:
        e.close()
    eng = engine6(2)
    b0 = eng.info()["device_bytes"]
    raises(GS_ERANGE, lambda: eng.enable_cluster_view(groups=[1, 1], weights=[1, wmax + 1]), "group 1")
    raises(GS_ERANGE, lambda: eng.enable_cluster_view(groups=[2], weights=[2**31, 2**31]), "group 0")
    # a refused enable leaves no view and no extra bytes
    assert eng.info()["device_bytes"] == b0
    raises(GS_ESTATE, eng.cluster_groups)
    raises(GS_ESTATE, lambda: eng.cluster_load(0))
    eng.enable_cluster_view(groups=[1, 1], weights=[1, wmax])  # and the bound itself enables
    eng.close()


def raw_enable(eng, groups, n_groups, weights=None):
    g = None if groups is None else np.ascontiguousarray(groups, dtype=np.uint32)
    w = None if weights is None else np.ascontiguousarray(weights, dtype=np.uint32)
    gs._check(gs.lib().gs_cluster_enable_groups(eng.h, None if g is None else gs._ptr(g), n_groups,
                                                None if w is None else gs._ptr(w)))


def test_arguments_and_states():
    eng = engine6()
    b0 = eng.info()["device_bytes"]
    # GS_EINVAL, naming the argument (past the Python mirror's own checks)
    raises(GS_EINVAL, lambda: raw_enable(eng, [3, 1, 2], 3), "group_slots")       # sums to 6
    raises(GS_EINVAL, lambda: raw_enable(eng, [3, 1, 4], 3), "group_slots")       # sums to 8
    raises(GS_EINVAL, lambda: raw_enable(eng, [3, 0, 4], 3), "group_slots[1]")    # an empty group
    raises(GS_EINVAL, lambda: raw_enable(eng, [1] * 8, 8), "n_groups")            # more groups than slots
    raises(GS_EINVAL, lambda: raw_enable(eng, [7], 0), "n_groups")
    raises(GS_EINVAL, lambda: raw_enable(eng, None, 3), "group_slots")
    assert eng.info()["device_bytes"] == b0
    for read in (eng.cluster_load, eng.cluster_rounds, eng.cluster_groups, lambda: eng.cluster_load(0)):
        raises(GS_ESTATE, read)
    # one group per table on an engine without tables: one group
    eng.enable_cluster_view(groups="tables")
    gsz, w = eng.cluster_groups()
    assert gsz.tolist() == [S1] and w.tolist() == [1] * S1
    eng.enable_cluster_view()            # G = 1 with unit weights and gs_cluster_enable's view: the same grouping
    eng.enable_cluster_view(groups=[S1])
    eng.enable_cluster_view(weights=[1] * S1)
    raises(GS_ESTATE, lambda: eng.enable_cluster_view(groups=GROUPS1))
    raises(GS_ESTATE, lambda: eng.enable_cluster_view(weights=WEIGHTS1))
    eng.enable_cluster_view(False)
    assert eng.info()["device_bytes"] == b0
    eng.enable_cluster_view()            # the ungrouped view, read back as one unit group
    gsz, w = eng.cluster_groups()
    assert gsz.tolist() == [S1] and w.tolist() == [1] * S1
    eng.enable_cluster_view(groups=[S1])  # a no-op over it
    raises(GS_ESTATE, lambda: eng.enable_cluster_view(groups=GROUPS1))
    cnt = C.c_uint32(99)
    assert gs.lib().gs_cluster_groups(eng.h, None, 0, C.byref(cnt), None) == GS_ERANGE and cnt.value == 1
    eng.enable_cluster_view(False)
    eng.enable_cluster_view(groups=GROUPS1, weights=WEIGHTS1)
    eng.enable_cluster_view(groups=GROUPS1, weights=WEIGHTS1)  # the identical grouping again: a no-op
    b1 = eng.info()
    assert b1["device_bytes"] >= b0 + 3 * 68 * N1
    raises(GS_ESTATE, lambda: eng.enable_cluster_view())                       # gs_cluster_enable(e, 1) over it
    raises(GS_ESTATE, lambda: eng.enable_cluster_view(groups=GROUPS1))         # other weights
    raises(GS_ESTATE, lambda: eng.enable_cluster_view(groups=[3, 2, 2], weights=WEIGHTS1))  # another grouping
    raises(GS_ESTATE, lambda: eng.enable_cluster_view(groups="tables", weights=WEIGHTS1))
    assert eng.info()["device_bytes"] == b1["device_bytes"]
    gsz, w = eng.cluster_groups()
    assert gsz.dtype == w.dtype == np.uint32 and gsz.tolist() == GROUPS1 and w.tolist() == WEIGHTS1
    cnt = C.c_uint32(0)
    two = np.zeros(2, dtype=np.uint32)
    assert gs.lib().gs_cluster_groups(eng.h, gs._ptr(two), 2, C.byref(cnt), None) == GS_ERANGE and cnt.value == 3
    raises(GS_EINVAL, eng.cluster_load)        # the un-suffixed reads at G > 1
    raises(GS_EINVAL, eng.cluster_rounds)
    raises(GS_EINVAL, lambda: eng.cluster_load(3))   # g >= G
    raises(GS_EINVAL, lambda: eng.cluster_rounds(3))
    assert all(not v.any() for g in range(3) for v in eng.cluster_load(g).values())
    eng.enable_cluster_view(False)             # gs_cluster_enable(e, 0) frees a grouped view too
    assert eng.info()["device_bytes"] == b0
    eng.close()
    _, st = synth.network(N1)
    part = gs.Engine(st, S1, seed=23, active_set_size=12, rotation_probability=0.1, part=(0, 1))
    raises(GS_ESTATE, lambda: part.enable_cluster_view(groups=GROUPS1))
    raises(GS_ESTATE, lambda: part.enable_cluster_view(groups="tables"))
    part.close()


def test_lifecycle():
    eng = engine6()
    b0 = eng.info()
    eng.set_slots(ORIGINS1)
    eng.init_active_sets()
    eng.round(0, record=True)  # a recorded round before the view exists
    assert eng.info()["device_bytes"] == b0["device_bytes"]
    eng.enable_cluster_view(groups=GROUPS1, weights=WEIGHTS1)
    b1 = eng.info()
    assert b1["other_bytes"] - b0["other_bytes"] == b1["device_bytes"] - b0["device_bytes"] >= 3 * 68 * N1
    assert b1["pair_bytes"] == b0["pair_bytes"]
    for g in range(3):  # the round recorded before enable reads as a zero entry in every group
        cr = eng.cluster_rounds(g)
        assert len(cr) == 1 == len(eng.summaries()) and cr.tobytes() == bytes(cr.nbytes)
        assert all(not v.any() for v in eng.cluster_load(g).values())
    eng.round(1, record=False)
    assert all(len(eng.cluster_rounds(g)) == 1 and not eng.cluster_load(g)["egress"].any() for g in range(3))
    eng.round(2, record=True)
    sm = eng.summaries()
    for g, (lo, hi) in enumerate([(0, 3), (3, 4), (4, 7)]):
        cr = eng.cluster_rounds(g)
        assert len(cr) == 2 and cr[:1].tobytes() == bytes(cr[:1].nbytes)
        assert int(cr[1]["pushes"]) == sum(WEIGHTS1[j] * int(sm[1][j]["pushes"]) for j in range(lo, hi)) > 0
    eng.set_slots(ORIGINS1)  # zeroes every group's totals, peaks and round list
    for g in range(3):
        assert all(not v.any() for v in eng.cluster_load(g).values()) and len(eng.cluster_rounds(g)) == 0
    eng.init_active_sets()
    eng.round(0, record=True)
    assert all(len(eng.cluster_rounds(g)) == 1 and eng.cluster_load(g)["egress_peak"].any() for g in range(3))
    eng.enable_cluster_view(False)
    assert eng.info()["device_bytes"] == b0["device_bytes"]
    raises(GS_ESTATE, lambda: eng.cluster_load(0))
    eng.round(1, record=True)  # and rounds go on without it
    assert len(eng.summaries()) == 2
    eng.close()


# --- 7. whole simulations ------------------------------------------------------------------------
def test_whole_simulations_by_table():
    n, iters, warm, seed, p = 60, 30, 5, 11, 0.1
    ranks, aszs, weights = [1, 2, 7, 30, 3], [12, 4, 12, 4, 12], [3, 1, 0, 2, 5]
    _, st = synth.network(n)
    kw = dict(n_sims=5, origin_ranks=ranks, iterations=iters, warm_up=warm, p=p, seed=seed, test_type=6, aszs=aszs)
    res = gs.run_simulations(st, cluster="tables", cluster_weights=weights, **kw)
    ref = gs.run_simulations(st, **kw)
    for s in range(5):  # every other name reads what it reads without the view
        for nm in tv.F64_NAMES:
            assert res.f64(s, nm).tobytes() == ref.f64(s, nm).tobytes(), nm
        for nm in tv.U64_NAMES:
            assert np.array_equal(res.u64(s, nm), ref.u64(s, nm)), nm
    # the same engine by hand: the tables in the order of their first sim, the sims in table order
    desc = np.sort(st)[::-1]
    origins = [int(np.nonzero(st == desc[r - 1])[0][0]) for r in ranks]
    order = [0, 2, 4, 1, 3]  # sims of size 12, then of size 4
    eng = gs.Engine(st, 5, fanout=6, seed=seed, trajectories=[(12, p, 3), (4, p, 2)])
    eng.set_slots([origins[i] for i in order], min_ingress=2, thresholds=0.15)
    eng.enable_cluster_view(groups="tables", weights=[weights[i] for i in order])
    eng.init_active_sets()
    for it in range(iters):
        eng.round(it, record=it >= warm)
    for s in range(5):  # the names under a sim answer with its own group's arrays
        g = 0 if aszs[s] == 12 else 1
        load, cr = eng.cluster_load(g), eng.cluster_rounds(g)
        assert len(cr) == iters - warm
        for k in TOTALS + PEAKS:
            assert np.array_equal(res.u64(s, "cluster_" + k), load[k].astype(np.uint64)), (s, k)
        for k in ("pushes", "egress_max", "egress_max_node", "ingress_max", "ingress_max_node", "senders"):
            assert np.array_equal(res.u64(s, "cluster_round_" + k), cr[k].astype(np.uint64)), (s, k)
    assert eng.cluster_load(0)["egress"].sum() > 0 and eng.cluster_load(1)["delivered"].sum() > 0
    assert not np.array_equal(res.u64(0, "cluster_egress"), res.u64(1, "cluster_egress"))
    eng.close()
