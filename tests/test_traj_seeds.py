"""A Philox seed per trajectory table (gs_create_traj_seeds): table t draws INIT, ROTATE, DECIDE
and FAIL on its own key, so a slot of table t is bit-identical to a gs_create engine with that
seed, size and probability -- seed replicas, and sweeps x replicas, as one engine. Slot k is
compared, bit for bit and round by round, with an oracle sim built with the slot's own seed
and fanout and run with its table's size and probability.

Each case's oracle trace is computed once and shared by the tests that run it. The cases
(synth.network, threshold 0.15, min-ingress 2; a table is (size, probability, seed), a slot is
(table, origin rank, fanout)) and the prunes each slot emits over the case's rounds in the
oracle alone, recorded from a CPU run and asserted in the trace so that no case passes on an
idle prune path. Each trace also asserts, from the oracle alone, that what the seeds must
separate really differs: the initial entries of two tables of equal size, and (with failures)
the failed sets of two seeds at equal fraction -- one shared key or one shared array of fail
ranks cannot pass.
  S1  200 nodes, three tables of size 12 at seeds 7 / 8 / 9, two slots each (the one-kernel round
      with rotation ahead per key, the step-wise calls, the split round, GS_ROT_AHEAD=0)
  S2  150 nodes, seeds x sizes x per-slot fanouts (the PF kernels composed with MT; the fanout-1
      slot prunes nothing, as in test_traj's case C)
  S3  180 nodes, sizes 4 / 16 at seeds 11 / 12 each, fail-nodes at round 2 (fail ranks per table in
      the round kernel's prepass, the stats pass, the readback)
  M1  300 nodes on the multi-source BFS, sizes 12 / 20 at seeds 5 / 6, eight slots in one group,
      fail-nodes at round 2 (failure classes per table: own rows and the lower-bucket path)
  M2  M1's tables with 30 slots: a table straddles the group boundary (28 + 2)
"""
import functools
import hashlib

import numpy as np
import pytest

import engine_bind as eb
import oracle_bind as ob
import test_traj as tt

gs = eb.gs
pytestmark = pytest.mark.gpu
U64MAX = np.uint64(2**64 - 1)
THR, MI = 0.15, 2
MULTI = dict(bfs_mode=gs.GS_BFS_MULTI, traj_multi=True)
FULL_EVERY = 5

_M_TABLES = [(12, .05, 5), (20, .05, 5), (12, .05, 6), (20, .05, 6)]
CASES = {
    "S1": dict(n=200, rounds=30, tables=[(12, .05, 7), (12, .05, 8), (12, .05, 9)],
               slots=[(0, 1, 6), (0, 40, 6), (1, 1, 6), (1, 40, 6), (2, 1, 6), (2, 40, 6)],
               prunes=[987, 992, 987, 989, 990, 991]),
    "S2": dict(n=150, rounds=30, tables=[(7, .05, 3), (12, .05, 3), (12, .05, 4)],
               slots=[(0, 1, 1), (0, 4, 3), (0, 9, 7), (1, 1, 2), (1, 4, 9), (1, 9, 12), (2, 1, 2), (2, 4, 9),
                      (2, 9, 12)],
               prunes=[0, 306, 896, 175, 1194, 1638, 141, 1172, 1610]),
    "S3": dict(n=180, rounds=30, tables=[(4, .03, 11), (4, .03, 12), (16, .03, 11), (16, .03, 12)],
               slots=[(0, 1, 4), (0, 3, 3), (1, 1, 4), (1, 3, 3), (2, 5, 6), (2, 9, 16), (3, 5, 6), (3, 9, 16)],
               fail_at=2, fractions=[.1, .2, .1, .2, .3, .5, .3, .5],
               prunes=[416, 222, 391, 194, 554, 1273, 551, 1257]),
    "M1": dict(n=300, rounds=26, tables=_M_TABLES,
               slots=[(0, 1, 6), (0, 150, 6), (1, 1, 6), (1, 40, 6), (2, 1, 6), (2, 150, 6), (3, 1, 6), (3, 90, 6)],
               fail_at=2, fractions=[.1, .25, .1, .25, .1, .25, .1, .25],
               prunes=[1361, 1037, 1361, 1031, 1318, 1046, 1318, 1085]),
    "M2": dict(n=300, rounds=22, tables=_M_TABLES, light=True,
               slots=[(0, r, 6) for r in (1, 2, 5, 20, 60, 120, 200, 250)] +
                     [(1, r, 6) for r in (1, 3, 10, 40, 90, 150, 260, 300)] +
                     [(2, r, 6) for r in (1, 4, 7, 15, 30, 75, 130, 180)] +
                     [(3, r, 6) for r in (1, 6, 12, 25, 50, 100)],  # slots 24..29: groups of 28 + 2
               prunes=[1518, 1518, 1518, 1521, 1519, 1526, 1524, 1519, 1518, 1518, 1516, 1522, 1516, 1524, 1521, 1520,
                       1473, 1476, 1477, 1484, 1486, 1487, 1474, 1475, 1473, 1483, 1484, 1487, 1486, 1486]),
}


def trajectories(c):
    """The engine's tables (size, probability, slots, seed): the case's slots are grouped by table."""
    tabs = [t for t, _, _ in c["slots"]]
    assert tabs == sorted(tabs)
    return [(a, p, tabs.count(t), sd) for t, (a, p, sd) in enumerate(c["tables"])]


@functools.lru_cache(maxsize=None)
def trace(name):
    """The oracle's state after every step of every round of a case: one sim per slot, built with
    the slot's own seed and fanout and run with its table's size and probability. light: hops,
    prunes and counters per round, the rest in the last round only."""
    c = CASES[name]
    n, rounds, light = c["n"], c["rounds"], c.get("light", False)
    pks, st = eb.synth.network(n)
    tab = [t for t, _, _ in c["slots"]]
    sims = [ob.Sim(ob.PHILOX, c["tables"][t][2], pks, st, f) for t, _, f in c["slots"]]
    origins = [sims[0].find_nth_largest(r) for _, r, _ in c["slots"]]
    size = [c["tables"][t][0] for t in tab]
    prob = [c["tables"][t][1] for t in tab]
    first = [tab.index(t) for t in range(len(c["tables"]))]  # a sim of each table
    for s, a in zip(sims, size):
        s.init_philox(a)
    out = dict(st=st, pks=pks, origins=origins, rounds=[],
               entries0=[sims[k].entries(c["tables"][t][0]) for t, k in enumerate(first)])
    # what the seeds must separate: tables of equal size and different seed start from different entries
    sep = 0
    for t, (a, _, sd) in enumerate(c["tables"]):
        for u, (b, _, se) in enumerate(c["tables"][:t]):
            if a == b and sd != se:
                assert not np.array_equal(out["entries0"][t][0], out["entries0"][u][0]), (name, t, u)
                sep += 1
    assert sep > 0, name
    totals = [0] * len(sims)
    for r in range(rounds):
        last = r == rounds - 1
        full = last if light else (r % FULL_EVERY == 0 or last)
        rec = dict(full=full, slots=[])
        if c.get("fail_at") == r:
            for s, f in zip(sims, c["fractions"]):
                s.fail_nodes(f)
            rec["failed"] = [np.asarray(s.failed()) for s in sims]
            sep = 0  # ... and two seeds at equal fraction fail different nodes (equal seeds: nested sets)
            for k in range(len(sims)):
                for j in range(k):
                    if c["fractions"][j] != c["fractions"][k]:
                        continue
                    same = np.array_equal(rec["failed"][j], rec["failed"][k])
                    if c["tables"][tab[j]][2] != c["tables"][tab[k]][2]:
                        assert not same and rec["failed"][k].sum() > 0, (name, j, k)
                        sep += 1
                    else:
                        assert same, (name, j, k)
            assert sep > 0, name
        for k, (s, o) in enumerate(zip(sims, origins)):
            q = {}
            s.run_gossip(o)
            q["dist"] = s.distances()
            if not light:
                q["orders"] = s.orders_all(64 * n)
            if full and not light:
                q["mst"] = {u: sorted(m) for u in range(n) for m in [s.mst(u)] if m}
            s.consume_messages(o)
            s.send_prunes(o, THR, MI)
            q["prunes"] = s.prunes()
            totals[k] += len(q["prunes"])
            if full:
                q["caches"] = s.caches(o)
            s.prune_connections()
            q["counters"] = tuple(np.where(a == U64MAX, 0, a) for a in s.counters())
            q["pruned"] = s.pruned_all(o)
            s.chance_to_rotate(size[k], prob[k], r)
            if full:
                q["pruned_rot"] = s.pruned_all(o)
            rec["slots"].append(q)
        if full:
            rec["entries"] = [sims[k].entries(c["tables"][t][0]) for t, k in enumerate(first)]
        out["rounds"].append(rec)
    out["totals"] = totals
    assert totals == c["prunes"], (name, totals)  # (no case passes on an idle prune path)
    return out


def make_engine(name, **kw):
    c, t = CASES[name], trace(name)
    fanouts = [f for _, _, f in c["slots"]]
    # (seed=12345: unused once every table carries its own)
    eng = gs.Engine(t["st"], len(c["slots"]), fanout=max(fanouts), seed=12345, trajectories=trajectories(c), **kw)
    assert eng.table_seeds() == [sd for _, _, sd in c["tables"]]
    assert eng.trajectories() == [tr[:3] for tr in trajectories(c)]
    eng.set_slots(t["origins"], MI, THR)
    if len(set(fanouts)) > 1:
        eng.set_slot_fanouts(fanouts)
    eng.init_active_sets()
    return eng


def _failed_of(t, c, upto):
    """Each slot's failed set after round `upto`'s fail_nodes, or none."""
    at = c.get("fail_at")
    if at is None or upto < at:
        return [np.zeros(c["n"], dtype=bool)] * len(c["slots"])
    return [f.astype(bool) for f in t["rounds"][at]["failed"]]


def run_rounds(name, **kw):
    """gs_round (the one-kernel round, the step kernels with split_round, or the multi-source BFS's
    round) against the trace."""
    c, t = CASES[name], trace(name)
    eng = make_engine(name, **kw)
    S = len(c["slots"])
    tt.assert_entries(eng, t["entries0"])
    for r, rec in enumerate(t["rounds"]):
        if "failed" in rec:
            eng.fail_nodes(c["fractions"])
            for k in range(S):
                np.testing.assert_array_equal(eng.failed(k), rec["failed"][k], err_msg=f"{name} failed set slot {k}")
        eng.round(r, record=True)
        for k, q in enumerate(rec["slots"]):
            msg = f"{name} slot {k} {c['slots'][k]} round {r}"
            np.testing.assert_array_equal(eng.distances(k), q["dist"], err_msg="hops " + msg)
            assert eng.prunes(k) == q["prunes"], "prunes " + msg
            for got, want in zip(eng.counters(k), q["counters"]):
                np.testing.assert_array_equal(got, want, err_msg="counters " + msg)
            if rec["full"]:
                tt.assert_caches(eng, k, q["caches"], "caches " + msg)
                np.testing.assert_array_equal(eng.pruned_all(k), q["pruned_rot"], err_msg="prune state " + msg)
        if rec["full"]:
            tt.assert_entries(eng, rec["entries"])
            summ = eng.summaries()
            assert summ.shape == (r + 1, S)
            for rr in range(r + 1):
                failed = _failed_of(t, c, rr)
                for k, q in enumerate(t["rounds"][rr]["slots"]):
                    unreached = q["dist"] == U64MAX
                    assert int(summ[rr, k]["visited"]) == int((~unreached).sum())
                    assert int(summ[rr, k]["prunes"]) == len(q["prunes"])
                    # stranded = unreached and not failed, on the slot's own table's fail ranks
                    assert int(summ[rr, k]["stranded"]) == int((unreached & ~failed[k]).sum()), (name, rr, k)
                    if "orders" in q:
                        assert int(summ[rr, k]["pushes"]) == len(q["orders"][1])
    return eng


# ------------------------------------------------ the workgroup engine ----
def test_s1_fused_round():
    eng = run_rounds("S1")
    assert eng.info()["fused_round"] and eng.info()["bfs_mode"] == gs.GS_BFS_WORKGROUP


def test_s1_split_round():
    eng = run_rounds("S1", split_round=True)
    assert not eng.info()["fused_round"]


def test_s1_standalone_rotation(monkeypatch):
    """GS_ROT_AHEAD=0: the rotation launches of every table on its key and the round kernel's
    deferred clear per table."""
    monkeypatch.setenv("GS_ROT_AHEAD", "0")  # (read when the engine is created)
    eng = run_rounds("S1")
    assert eng.info()["fused_round"]


def test_s1_stepwise_round():
    """run_gossip ... chance_to_rotate, with the inbound lists and mst of every slot."""
    name = "S1"
    c, t = CASES[name], trace(name)
    n = c["n"]
    eng = make_engine(name)
    tt.assert_entries(eng, t["entries0"])
    for r, rec in enumerate(t["rounds"]):
        eng.run_gossip()
        for k, q in enumerate(rec["slots"]):
            msg = f"{name} slot {k} {c['slots'][k]} round {r}"
            np.testing.assert_array_equal(eng.distances(k), q["dist"], err_msg="hops " + msg)
            off, src, hop = eng.inbound(k)
            ooff, osrc, ohop = q["orders"]
            np.testing.assert_array_equal(off, ooff, err_msg="inbound " + msg)
            np.testing.assert_array_equal(src[:off[n]], osrc, err_msg="inbound " + msg)
            np.testing.assert_array_equal(hop[:off[n]], ohop, err_msg="inbound " + msg)
            if rec["full"]:
                assert eng.mst(k) == q["mst"], "mst " + msg
        eng.consume_messages()
        eng.send_prunes()
        for k, q in enumerate(rec["slots"]):
            msg = f"{name} slot {k} round {r}"
            assert eng.prunes(k) == q["prunes"], "prunes " + msg
            if rec["full"]:
                tt.assert_caches(eng, k, q["caches"], "caches " + msg)
        eng.prune_connections()
        for k, q in enumerate(rec["slots"]):
            for got, want in zip(eng.counters(k), q["counters"]):
                np.testing.assert_array_equal(got, want, err_msg=f"counters {name} slot {k} round {r}")
            np.testing.assert_array_equal(eng.pruned_all(k), q["pruned"], err_msg=f"prune state {name} {k} round {r}")
        eng.chance_to_rotate(r)
        if rec["full"]:
            tt.assert_entries(eng, rec["entries"])
            for k, q in enumerate(rec["slots"]):
                np.testing.assert_array_equal(eng.pruned_all(k), q["pruned_rot"])


def test_s2_seeds_sizes_and_slot_fanouts():
    eng = run_rounds("S2")
    assert eng.info()["fused_round"]
    np.testing.assert_array_equal(eng.slot_fanouts(), [f for _, _, f in CASES["S2"]["slots"]])


@pytest.mark.parametrize("split", [False, True])
def test_s3_fail_nodes_per_table(split):
    """The failed sets per slot against the oracle (gs_read_failed reads the slot's own table's
    ranks), the round kernel's prepass on them, and `stranded` in the summaries: in the one-kernel
    round, and with split_round through the stand-alone stats pass."""
    eng = run_rounds("S3", split_round=split)
    assert eng.info()["fused_round"] == (not split)


# ------------------------------------------------ the multi-source BFS ----
def _is_multi(eng):
    info = eng.info()
    return info["bfs_mode"] == gs.GS_BFS_MULTI and not info["fused_round"]


def test_m1_persistent_loop():
    c, t = CASES["M1"], trace("M1")
    # rank 1 under every table; rank 150 (a low-bucket origin) under two tables
    assert len({t["origins"][k] for k in (0, 2, 4, 6)}) == 1 and t["origins"][1] == t["origins"][5]
    eng = run_rounds("M1", **MULTI)
    assert _is_multi(eng) and eng.info()["bfs_persistent"] and eng.bfs_geometry()["groups"] == 1


def test_m1_launched_loop(monkeypatch):
    monkeypatch.setenv("GS_MV_PBFS", "0")  # (read when the engine is created)
    eng = run_rounds("M1", **MULTI)
    assert _is_multi(eng) and not eng.info()["bfs_persistent"]


def test_m2_table_straddling_the_group_boundary():
    eng = run_rounds("M2", **MULTI)
    geo = eng.bfs_geometry()
    assert _is_multi(eng) and geo["group_width"] == 28 and geo["groups"] == 2
    assert min(trace("M2")["totals"]) > 0


# ------------------------------------------------ engine-level properties ----
def _digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


@pytest.mark.parametrize("kw", [{}, MULTI], ids=["workgroup", "multi"])
def test_equal_seeds_change_nothing(kw):
    """gs_create_traj_seeds with all seeds equal is the gs_create_traj engine at that seed: the
    per-slot digests of hops, prune state, caches and summaries over 25 rounds, and the memory."""
    _, st = eb.synth.network(240)
    tabs, origins, S, rounds = [(8, .05, 2), (12, .05, 1), (12, .2, 2)], [3, 77, 150, 239, 3], 5, 25

    def run(eng):
        eng.set_slots(origins, MI, THR)
        eng.init_active_sets()
        eng.fail_nodes([0, .1, 0, .2, .1])
        out = []
        for r in range(rounds):
            eng.round(r, record=True)
            out.append([_digest(eng.hops(k), eng.pruned_all(k), *eng.caches(k)) for k in range(S)])
        summ = eng.summaries()
        return out, [_digest(summ[:, k]) for k in range(S)], int(summ["prunes"].sum()), [eng.failed(k) for k in range(S)]

    a = gs.Engine(st, S, fanout=6, seed=999, trajectories=[(x, p, k, 21) for x, p, k in tabs], **kw)
    b = gs.Engine(st, S, fanout=6, seed=21, trajectories=tabs, **kw)
    assert a.table_seeds() == b.table_seeds() == [21, 21, 21]
    assert a.trajectories() == b.trajectories() == tabs
    ia, ib = a.info(), b.info()
    assert ia == ib  # (device, pair and other bytes: gs_engine_memory)
    ra, rb = run(a), run(b)
    assert ra[2] > 0
    assert ra[0] == rb[0] and ra[1] == rb[1]
    for x, y in zip(ra[3], rb[3]):
        np.testing.assert_array_equal(x, y)
    # keys that differ cost a rank array per table (counted under other_bytes), nothing per pair
    c = gs.Engine(st, S, fanout=6, trajectories=[(x, p, k, 21 + t) for t, (x, p, k) in enumerate(tabs)], **kw)
    ic = c.info()
    assert ic["pair_bytes"] == ia["pair_bytes"] and ic["other_bytes"] > ia["other_bytes"]
    # one table with a seed is gs_create at that seed
    d = gs.Engine(st, 2, fanout=6, seed=5, trajectories=[(12, .05, 2, 21)], **kw)
    e = gs.Engine(st, 2, fanout=6, seed=21, active_set_size=12, rotation_probability=.05,
                  bfs_mode=kw.get("bfs_mode", gs.GS_BFS_WORKGROUP))
    assert d.table_seeds() == e.table_seeds() == [21] and d.info() == e.info()
    for x in (d, e):
        x.set_slots([3, 77], MI, THR)
        x.init_active_sets()
        for r in range(5):
            x.round(r)
    for k in range(2):
        np.testing.assert_array_equal(d.hops(k), e.hops(k))
    for x, y in zip(d.active_sets(), e.active_sets()):
        np.testing.assert_array_equal(x, y)


def test_refusals_and_round_trip():
    import ctypes as C
    _, st = eb.synth.network(100)
    tr = [(12, .25, 1, 5), (8, .5, 2, 6)]

    def make(tr=tr, n_slots=3, **kw):
        return gs.Engine(st, n_slots, fanout=6, seed=1, trajectories=tr, **kw)

    for mode in (gs.GS_BFS_LEVEL, gs.GS_BFS_BINNED, gs.GS_BFS_HYBRID):
        for flag in (False, True):
            with pytest.raises(gs.GsError) as ei:
                make(bfs_mode=mode, traj_multi=flag)
            assert ei.value.code == -1
    with pytest.raises(gs.GsError) as ei:  # MULTI without the flag stays refused
        make(bfs_mode=gs.GS_BFS_MULTI)
    assert ei.value.code == -1 and "GS_BFS_WORKGROUP" in str(ei.value)
    for bad in ([(12, .1, 3, 5), (8, .1, 0, 6)], [(0, .1, 1, 5), (12, .1, 2, 6)], [(12, 1.5, 1, 5), (12, .1, 2, 6)],
                [(12, .1, 1, 5), (8, .1, 1, 6)]):
        with pytest.raises(gs.GsError) as ei:
            make(bad)
        assert ei.value.code == -1, bad
    for mixed in ([(12, .25, 1, 5), (8, .5, 2)], [(12, .25, 1), (8, .5, 2, 6)]):
        with pytest.raises(ValueError):
            make(mixed)
    eng = make()
    assert eng.table_seeds() == [5, 6] and eng.trajectories() == [(12, .25, 1), (8, .5, 2)]
    assert eng.info()["bfs_mode"] == gs.GS_BFS_WORKGROUP and eng.info()["fused_round"]
    # gs_engine_traj_seeds with a short buffer: GS_ERANGE and the count
    buf, n = (C.c_uint64 * 2)(), C.c_uint32()
    assert gs.lib().gs_engine_traj_seeds(eng.h, C.cast(buf, C.c_void_p), 1, C.byref(n)) == -4 and n.value == 2
    assert gs.lib().gs_engine_traj_seeds(eng.h, C.cast(buf, C.c_void_p), 2, C.byref(n)) == 0 and list(buf) == [5, 6]
    # the un-suffixed entry calls stay GS_EINVAL on several tables
    eng.set_slots([1, 2, 3], MI, THR)
    eng.init_active_sets()
    for call in (eng.active_sets, lambda: eng.get_entry(3, 0), lambda: eng.set_entry(3, 0, [1, 2])):
        with pytest.raises(gs.GsError) as ei:
            call()
        assert ei.value.code == -1 and "_traj" in str(ei.value)
    # an engine made another way reports its seed for every table
    plain = gs.Engine(st, 2, seed=17)
    assert plain.table_seeds() == [17]
    tabs = gs.Engine(st, 3, seed=17, trajectories=[(12, .25, 1), (8, .5, 2)])
    assert tabs.table_seeds() == [17, 17]
    # seeds == NULL through the C ABI is gs_create_traj
    p = gs.Params(6, 12, 0., 23, 0, gs.GS_BFS_AUTO, 0, 0)
    arr = (gs.Traj * 2)(gs.Traj(12, .1, 1), gs.Traj(8, .1, 2))
    h = C.c_void_p()
    stc = np.ascontiguousarray(st, dtype=np.uint64)
    assert gs.lib().gs_create_traj_seeds(C.byref(p), stc.ctypes.data_as(C.c_void_p), len(stc), 3,
                                         C.cast(arr, C.c_void_p), 2, None, C.byref(h)) == 0
    assert gs.lib().gs_engine_traj_seeds(h, C.cast(buf, C.c_void_p), 2, C.byref(n)) == 0 and list(buf) == [23, 23]
    gs.lib().gs_destroy(h)


# ------------------------------------------------------------- whole sims ----
import gossip_sim_amd.sweep as sw  # noqa: E402

ITER, WARM = 50, 30  # 30 warm-up + 20 measured rounds: cache entries reach their 20th upsert and prune


def _assert_same(a, i, b, j, msg):
    for kind, name in sw.NAMES:
        x = a.f64(i, name) if kind == "f" else a.u64(i, name)
        y = b.f64(j, name) if kind == "f" else b.u64(j, name)
        np.testing.assert_array_equal(x, y, err_msg=f"{msg} {name}")


def test_run_simulations_with_seeds():
    """Sims 0 and 2 share a seed but not a size; 0, 1, 3 share a size but not a seed."""
    _, st = eb.synth.network(200)
    seeds, aszs = [1, 2, 1, 3], [12, 12, 16, 12]
    res = gs.run_simulations(st, n_sims=4, seeds=seeds, aszs=aszs, p=.05, iterations=ITER, warm_up=WARM, seed=77)
    cov = []
    for k, (sd, a) in enumerate(zip(seeds, aszs)):
        one = gs.run_simulations(st, n_sims=1, seed=sd, asz=a, p=.05, iterations=ITER, warm_up=WARM)
        assert len(one.f64(0, "coverage")) == ITER - WARM and one.u64(0, "prune_hist").sum() > 0
        _assert_same(res, k, one, 0, f"sim {k}")
        cov.append(_digest(one.u64(0, "egress_hist"), one.u64(0, "ingress_hist"), one.f64(0, "rmr")))
    assert len(set(cov)) == 4  # (the four runs differ: nothing compares equal by default)
    # fail-nodes: every sim's failed set comes from its own key
    res = gs.run_simulations(st, n_sims=3, seeds=[1, 2, 1], fractions=[.2, .2, .3], p=.05, iterations=ITER,
                             warm_up=WARM, test_type=5, when_to_fail=2)
    for k, (sd, f) in enumerate(zip([1, 2, 1], [.2, .2, .3])):
        one = gs.run_simulations(st, n_sims=1, seed=sd, fractions=[f], p=.05, iterations=ITER, warm_up=WARM,
                                 test_type=5, when_to_fail=2)
        _assert_same(res, k, one, 0, f"fail-nodes sim {k}")
    # one distinct triple: that seed replaces the configuration's
    res = gs.run_simulations(st, n_sims=2, seeds=[4, 4], origin_ranks=[1, 9], p=.05, iterations=ITER, warm_up=WARM,
                             seed=77)
    one = gs.run_simulations(st, n_sims=2, seed=4, origin_ranks=[1, 9], p=.05, iterations=ITER, warm_up=WARM)
    for k in range(2):
        _assert_same(res, k, one, k, f"one triple sim {k}")


def test_run_trial_sweep_equals_per_unit_runs():
    _, st = eb.synth.network(200)
    sizes, seeds, calls = [12, 16], [1, 2, 3], []

    def runner(stakes, **kw):
        calls.append(kw["n_sims"])
        return gs.run_simulations(stakes, **kw)

    def cfg(a):
        return dict(asz=a, p=.05, iterations=ITER, warm_up=WARM)

    out = sw.run_trial_sweep(st, sizes, seeds, cfg, runner=runner)
    assert calls == [6] and out.n_sims == 6  # one engine
    for i, a in enumerate(sizes):
        for j, sd in enumerate(seeds):
            one = gs.run_simulations(st, n_sims=1, seed=sd, **cfg(a))
            for kind, name in sw.NAMES:
                want = one.f64(0, name) if kind == "f" else one.u64(0, name)
                np.testing.assert_array_equal(out.per_sim[i * len(seeds) + j][(kind, name)], want,
                                              err_msg=f"size {a} seed {sd} {name}")


# -------------------------------------------------------------------- CLI ----
from test_cli import F64_NAMES as CLI_F64, U64_NAMES as CLI_U64, cli, yaml_net  # noqa: E402,F401
import report_ref as rr  # noqa: E402


def test_cli_trials_batch_sweeps(yaml_net, tmp_path):
    """gossip-sim --trials 3 --batch-sweeps: one engine of three tables at seeds 13, 14, 15; its
    saved results equal three --seed runs', and the plan is one line with the seeds."""
    path = yaml_net[0]
    common = ["--accounts-from-yaml", "--account-file", path, "--iterations", ITER, "--warm-up-rounds", WARM,
              "-p", ".05"]
    res, plan = str(tmp_path / "g.txt"), str(tmp_path / "plan.txt")
    cli(*common, "--seed", 13, "--trials", 3, "--batch-sweeps", "--save-results", res, "--engine-plan", plan)
    assert open(plan).read().splitlines() == [
        "device 0 sims 0,1,2 active-set-size 12,12,12 fanouts 6,6,6 rotation-probability " +
        ",".join("%.17g" % float(".05") for _ in range(3)) + " seeds 13,14,15"]
    got = rr.read_results(res)
    assert len(got) == 3
    digests = set()
    for k in range(3):
        one = str(tmp_path / f"one{k}.txt")
        cli(*common, "--seed", 13 + k, "--save-results", one)
        (wf, wu), = rr.read_results(one)
        gf, gu = got[k]
        assert len(wf["coverage"]) == ITER - WARM
        for n in CLI_F64:
            np.testing.assert_array_equal(gf[n], wf[n], err_msg=f"trial {k} {n}")
        for n in CLI_U64:
            np.testing.assert_array_equal(gu[n], wu[n], err_msg=f"trial {k} {n}")
        digests.add(_digest(wu["egress_hist"], wu["ingress_hist"], wf["rmr"]))
    assert len(digests) == 3
