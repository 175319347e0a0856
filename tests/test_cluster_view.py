"""The cluster load view (gs_cluster_enable): per-node egress / ingress / prunes / deliveries
summed over every slot of an engine, on the device, per recorded round.

The oracle has no cross-slot view (one Cluster is one origin), so the expected values are built
here in numpy from the per-slot readbacks, which the parity tests pin to the oracle: after each
recorded round, Engine.counters(slot) (egress of an unreached node already reads 0) and
Engine.hops(slot) are summed over the slots into that round's E, I, P, D, H; totals, peaks and
the gs_cluster_round struct (np.argmax: the smallest id among equal maxima) accumulate from
them. Every comparison is exact equality.
"""
import numpy as np
import pytest

import engine_bind as eb

gs = eb.gs
synth = eb.synth
pytestmark = pytest.mark.gpu

GS_ESTATE = -5
TOTALS = ("egress", "ingress", "prunes", "delivered", "hop_sum")


class Expect:
    """The view's definition, restated over the per-slot readbacks."""

    def __init__(self, n):
        self.n = n
        self.tot = {k: np.zeros(n, dtype=np.uint64) for k in TOTALS}
        self.peak = {"egress_peak": np.zeros(n, dtype=np.uint32), "ingress_peak": np.zeros(n, dtype=np.uint32)}
        self.rounds = []
        self.unreached = 0  # (slot, node) pairs unreached in a recorded round

    def record(self, eng):
        r = {k: np.zeros(self.n, dtype=np.uint64) for k in TOTALS}
        for j in range(eng.n_slots):
            e, i, p = eng.counters(j)
            h = eng.hops(j).astype(np.uint64)
            d = (h >= 1) & (h <= 254)
            self.unreached += int((h == 0xFF).sum())
            r["egress"] += e
            r["ingress"] += i
            r["prunes"] += p
            r["delivered"] += d
            r["hop_sum"] += h * d
        for k in TOTALS:
            self.tot[k] += r[k]
        self.peak["egress_peak"] = np.maximum(self.peak["egress_peak"], r["egress"].astype(np.uint32))
        self.peak["ingress_peak"] = np.maximum(self.peak["ingress_peak"], r["ingress"].astype(np.uint32))
        self.rounds.append(dict(
            pushes=int(r["egress"].sum()), ingress=int(r["ingress"].sum()), prunes=int(r["prunes"].sum()),
            delivered=int(r["delivered"].sum()), egress_max=int(r["egress"].max()),
            egress_max_node=int(np.argmax(r["egress"])), ingress_max=int(r["ingress"].max()),
            ingress_max_node=int(np.argmax(r["ingress"])), senders=int((r["egress"] > 0).sum()), pad0=0))

    def check(self, eng, what=""):
        got = eng.cluster_load()
        for k in TOTALS:
            assert got[k].dtype == np.uint64 and np.array_equal(got[k], self.tot[k]), f"{what}: total {k}"
        for k, v in self.peak.items():
            assert got[k].dtype == np.uint32 and np.array_equal(got[k], v), f"{what}: {k}"
        cr = eng.cluster_rounds()
        assert len(cr) == len(self.rounds), f"{what}: {len(cr)} cluster rounds, {len(self.rounds)} recorded"
        assert len(cr) == len(eng.summaries()), f"{what}: cluster rounds and summaries differ in length"
        for r, exp in enumerate(self.rounds):
            for k, v in exp.items():
                assert int(cr[r][k]) == v, f"{what}: round {r} {k}: {int(cr[r][k])} != {v}"


def drive(eng, origins, rounds, *, first_recorded=0, fail_at=None, fractions=None, every=1, tag=""):
    """set_slots, the view on, init, `rounds` rounds (recorded from first_recorded on); the
    expectation is updated after every recorded round and compared every `every` of them."""
    ex = Expect(eng.n)
    eng.set_slots(origins)
    eng.enable_cluster_view()
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


# --- 1. every round path -----------------------------------------------------------------
N1, S1, ROUNDS1 = 131, 7, 26
ORIGINS1 = [0, 5, 17, 40, 77, 100, 130]
FRACTIONS1 = [0.0, 0.3, 0.0, 0.0, 0.3, 0.0, 0.0]
PATHS = {
    "wg_fused": dict(bfs_mode=gs.GS_BFS_WORKGROUP),
    "wg_fused_rotate_in_place": dict(bfs_mode=gs.GS_BFS_WORKGROUP, env={"GS_ROT_AHEAD": "0"}),
    "wg_split": dict(bfs_mode=gs.GS_BFS_WORKGROUP, split_round=True),
    "level": dict(bfs_mode=gs.GS_BFS_LEVEL),
    "binned": dict(bfs_mode=gs.GS_BFS_BINNED),
    "multi": dict(bfs_mode=gs.GS_BFS_MULTI),
    "multi_fused_consume": dict(bfs_mode=gs.GS_BFS_MULTI, env={"GS_MV_FUSED": "1"}),
    "hybrid": dict(bfs_mode=gs.GS_BFS_HYBRID),
}


def engine1(monkeypatch, path, **kw):
    opts = dict(PATHS[path])
    for k, v in opts.pop("env", {}).items():
        monkeypatch.setenv(k, v)
    _, st = synth.network(N1)
    return gs.Engine(st, S1, seed=23, active_set_size=12, rotation_probability=0.1, **opts, **kw)


@pytest.mark.parametrize("path", list(PATHS))
def test_every_round_path(monkeypatch, path):
    eng = engine1(monkeypatch, path)
    if path.startswith("wg_fused"):
        assert eng.info()["fused_round"]
    ex = drive(eng, ORIGINS1, ROUNDS1, first_recorded=2, fail_at=3, fractions=FRACTIONS1, tag=path)
    assert len(ex.rounds) == ROUNDS1 - 2  # rounds 0 and 1 do not count
    assert ex.tot["prunes"].sum() > 0, "no prune wave within the case's rounds: the prune path was idle"
    assert ex.unreached > 0, "every (slot, node) was reached in every recorded round: no stale egress byte"
    eng.close()


# --- 2. slot-split and node-block edges ----------------------------------------------------
EDGES = [("wg", 67, 70), ("level", 67, 70), ("wg", 67, 1), ("level", 67, 1), ("wg", 3, 3), ("level", 3, 3),
         ("multi", 1025, 5), ("level", 1025, 5)]


@pytest.mark.parametrize("mode,n,s", EDGES)
def test_slot_split_and_node_block_edges(mode, n, s):
    _, st = synth.network(n)
    bfs = {"wg": gs.GS_BFS_WORKGROUP, "level": gs.GS_BFS_LEVEL, "multi": gs.GS_BFS_MULTI}[mode]
    eng = gs.Engine(st, s, seed=5, active_set_size=12, rotation_probability=0.1, bfs_mode=bfs)
    ex = drive(eng, [j % n for j in range(s)], 8, every=4, tag=f"{mode} n={n} s={s}")
    assert len(ex.rounds) == 8 and ex.tot["egress"].sum() > 0
    eng.close()


# --- 3. table engines ------------------------------------------------------------------------
@pytest.mark.parametrize("seeded", [False, True])
@pytest.mark.parametrize("multi", [False, True])
def test_table_engines(seeded, multi):
    _, st = synth.network(N1)
    tables = [(4, 0.1, 3), (12, 0.0, 4)]
    if seeded:
        tables = [t + (sd,) for t, sd in zip(tables, (7, 8))]
    kw = dict(bfs_mode=gs.GS_BFS_MULTI, traj_multi=True) if multi else {}
    eng = gs.Engine(st, S1, seed=23, trajectories=tables, **kw)
    ex = drive(eng, ORIGINS1, 10, first_recorded=1, every=3, tag=f"tables seeded={seeded} multi={multi}")
    assert len(ex.rounds) == 9 and ex.tot["delivered"].sum() > 0
    eng.close()


# --- 4. the view changes nothing, and agrees with the accumulators -----------------------------
@pytest.mark.parametrize("path", ["wg_fused", "multi"])
def test_view_changes_nothing_and_matches_accumulators(monkeypatch, path):
    engs = [engine1(monkeypatch, path), engine1(monkeypatch, path)]
    for k, eng in enumerate(engs):
        eng.set_slots(ORIGINS1)
        if k == 0:
            eng.enable_cluster_view()
        eng.init_active_sets()
        for r in range(ROUNDS1):
            if r == 3:
                eng.fail_nodes(FRACTIONS1)
            eng.round(r, record=r >= 2)
    on, off = engs
    a, b = on.summaries(), off.summaries()
    assert a.shape == b.shape == (ROUNDS1 - 2, S1) and a.tobytes() == b.tobytes()
    sums = [np.zeros(N1, dtype=np.uint64) for _ in range(3)]
    for j in range(S1):
        x, y = on.accumulators(j), off.accumulators(j)
        for u, v in zip(x, y):
            assert np.array_equal(u, v), f"accumulators of slot {j}"
        for w in range(3):
            sums[w] += x[w]
    for u, v in zip(on.caches(0), off.caches(0)):
        assert np.array_equal(u, v)
    load = on.cluster_load()
    for w, k in enumerate(("egress", "ingress", "prunes")):
        assert np.array_equal(load[k], sums[w]), k
    assert load["prunes"].sum() > 0
    with pytest.raises(gs.GsError) as ei:
        off.cluster_load()
    assert ei.value.code == GS_ESTATE
    for eng in engs:
        eng.close()


# --- 5. the step-wise path ------------------------------------------------------------------
@pytest.mark.parametrize("mode", [gs.GS_BFS_WORKGROUP, gs.GS_BFS_MULTI])
def test_step_wise_record_round(mode):
    _, st = synth.network(N1)
    eng = gs.Engine(st, S1, seed=23, active_set_size=12, rotation_probability=0.1, bfs_mode=mode)
    ex = Expect(N1)
    eng.enable_cluster_view()  # (before set_slots: allowed whenever set_slots is)
    eng.set_slots(ORIGINS1)
    eng.init_active_sets()
    for r in range(24):
        eng.run_gossip()
        eng.consume_messages()
        eng.send_prunes()
        eng.prune_connections()
        eng.chance_to_rotate(r)
        if r >= 2:
            eng.record_round()
            ex.record(eng)
            if r % 5 == 0 or r == 23:
                ex.check(eng, f"step-wise round {r}")
    assert len(ex.rounds) == 22 and ex.tot["prunes"].sum() > 0
    eng.close()


# --- 6. lifecycle ----------------------------------------------------------------------------
def test_lifecycle():
    _, st = synth.network(N1)
    eng = gs.Engine(st, S1, seed=23, active_set_size=12, rotation_probability=0.1, bfs_mode=gs.GS_BFS_WORKGROUP)
    b0 = eng.info()
    for read in (eng.cluster_load, eng.cluster_rounds):
        with pytest.raises(gs.GsError) as ei:
            read()
        assert ei.value.code == GS_ESTATE
    eng.set_slots(ORIGINS1)
    eng.init_active_sets()
    eng.round(0, record=True)  # a recorded round before the view exists
    assert eng.info()["device_bytes"] == b0["device_bytes"], "the view costs memory before it is enabled"
    eng.enable_cluster_view()
    eng.enable_cluster_view()  # twice: a no-op
    b1 = eng.info()
    assert b1["device_bytes"] >= b0["device_bytes"] + 68 * N1
    assert b1["other_bytes"] - b0["other_bytes"] == b1["device_bytes"] - b0["device_bytes"]
    assert b1["pair_bytes"] == b0["pair_bytes"]
    load = eng.cluster_load()
    assert all(not v.any() for v in load.values())
    cr = eng.cluster_rounds()  # the round recorded before enable reads as a zero entry: indices stay aligned
    assert len(cr) == 1 == len(eng.summaries()) and cr.tobytes() == bytes(cr.nbytes)
    eng.round(1, record=False)
    assert len(eng.cluster_rounds()) == 1 and not eng.cluster_load()["egress"].any()  # not recorded: nothing counted
    eng.round(2, record=True)
    assert len(eng.cluster_rounds()) == 2 and eng.cluster_load()["egress"].sum() > 0
    assert int(eng.cluster_rounds()[1]["pushes"]) == int(eng.summaries()[1]["pushes"].sum())
    eng.set_slots(ORIGINS1)  # zeroes totals, peaks and the round list
    assert all(not v.any() for v in eng.cluster_load().values()) and len(eng.cluster_rounds()) == 0
    eng.init_active_sets()
    eng.round(0, record=True)
    assert len(eng.cluster_rounds()) == 1 and eng.cluster_load()["egress_peak"].any()
    eng.enable_cluster_view(False)
    assert eng.info()["device_bytes"] == b0["device_bytes"]
    with pytest.raises(gs.GsError) as ei:
        eng.cluster_load()
    assert ei.value.code == GS_ESTATE
    eng.round(1, record=True)  # and rounds go on without it
    assert len(eng.summaries()) == 2
    eng.close()

    part = gs.Engine(st, S1, seed=23, active_set_size=12, rotation_probability=0.1, part=(0, 1))
    with pytest.raises(gs.GsError) as ei:
        part.enable_cluster_view()
    assert ei.value.code == GS_ESTATE
    part.close()


# --- 7. whole simulations -------------------------------------------------------------------
F64_NAMES = ["coverage", "rmr", "branching", "hop_mean", "hop_median", "coverage_stats", "rmr_stats",
             "branching_stats", "aggregate_hops", "ldh", "stranded", "stranded_round_mean", "stranded_round_median"]
U64_NAMES = ["origin", "hop_max", "hop_min", "aggregate_hops", "ldh", "stranded", "stranded_times",
             "stranded_round_count", "stranded_round_max", "stranded_round_min", "hops_hist", "stranded_hist",
             "egress_hist", "ingress_hist", "prune_hist", "egress_cpb", "validator_hist", "hist_errors",
             "failed_count", "rmr_m", "rmr_n"]


def test_whole_simulations():
    n, ranks, iters, warm, seed, p = 60, [1, 2, 7, 30], 30, 5, 11, 0.1
    _, st = synth.network(n)
    kw = dict(n_sims=4, origin_ranks=ranks, iterations=iters, warm_up=warm, p=p, seed=seed, test_type=6)
    res = gs.run_simulations(st, cluster=True, **kw)
    ref = gs.run_simulations(st, **kw)
    for s in range(4):
        for nm in F64_NAMES:
            assert res.f64(s, nm).tobytes() == ref.f64(s, nm).tobytes(), nm
        for nm in U64_NAMES:
            assert np.array_equal(res.u64(s, nm), ref.u64(s, nm)), nm
        for nm in gs.CLUSTER_RESULT_NAMES:
            with pytest.raises(KeyError):
                ref.u64(s, nm)
    # the same engine by hand: origins = find_nth_largest_node (the lowest id holding the rank's stake)
    desc = np.sort(st)[::-1]
    origins = [int(np.nonzero(st == desc[r - 1])[0][0]) for r in ranks]
    assert origins == [int(res.u64(s, "origin")[0]) for s in range(4)]
    eng = gs.Engine(st, 4, fanout=6, active_set_size=12, rotation_probability=p, seed=seed)
    eng.set_slots(origins, min_ingress=2, thresholds=0.15)
    eng.enable_cluster_view()
    eng.init_active_sets()
    for it in range(iters):
        eng.round(it, record=it >= warm)
    load, cr = eng.cluster_load(), eng.cluster_rounds()
    assert len(cr) == iters - warm
    for s in (0, 3):  # the same arrays under any valid sim
        for k in TOTALS + ("egress_peak", "ingress_peak"):
            assert np.array_equal(res.u64(s, "cluster_" + k), load[k].astype(np.uint64)), k
        for k in ("pushes", "egress_max", "egress_max_node", "ingress_max", "ingress_max_node", "senders"):
            assert np.array_equal(res.u64(s, "cluster_round_" + k), cr[k].astype(np.uint64)), k
    assert load["egress"].sum() > 0 and load["delivered"].sum() > 0
    eng.close()
