"""Per-slot push fanout (gs_set_slot_fanouts): slot k of an engine created with
fanout = max(fanouts) is compared, bit for bit and round by round, with an oracle sim
built with fanouts[k] -- in every BFS strategy, the one-kernel round, whole sims, a
one-rank node-range partition and the CLI's batched push-fanout sweep.

Each case's oracle trace is computed once and shared by the strategies that run it.
The cases (synth.network, seed 7, threshold 0.15, min-ingress 2) and the prunes each
slot emits over the case's rounds in the oracle alone (fanout-1 slots: none, which is
asserted together with > 0 for every slot of fanout >= 2, so no case passes on an
idle prune path):
  A  240 nodes, fanouts 1,2,3,6,9,12 of active-set size 12: 0, 370, 643, 1329, 2046, 2744
  B  180 nodes, fail-nodes at round 2, fanouts 2,4,6,12:    105, 336, 539, 907
  C  200 nodes, active-set size 32 (u64 ring path):         0, 1179, 3792, 6139
  D  150 nodes, fanouts 1,3,7 of active-set size 7:         0, 297, 882
  E  120 nodes, 36 slots (two slot groups), fanouts 1 + k mod 12: >= 122 where fanout >= 2
"""
import ctypes as C
import functools

import numpy as np
import pytest

import engine_bind as eb
import oracle_bind as ob

gs = eb.gs
pytestmark = pytest.mark.gpu
U64MAX = np.uint64(2**64 - 1)
SEED, THR, MI = 7, 0.15, 2

CASES = {
    "A": dict(n=240, ranks=[1, 2, 7, 60, 240, 3], fanouts=[1, 2, 3, 6, 9, 12], asz=12, rounds=30, p=0.08,
              prunes=[0, 370, 643, 1329, 2046, 2744]),
    "A6": dict(n=240, ranks=[1, 2, 7, 60, 240, 3], fanouts=[1, 2, 3, 4, 5, 6], asz=12, rounds=30, p=0.08),
    "B": dict(n=180, ranks=[1, 3, 5, 9], fanouts=[2, 4, 6, 12], asz=12, rounds=30, p=0.03, fail_at=2,
              fractions=[0.1, 0.2, 0.3, 0.5], prunes=[105, 336, 539, 907]),
    "C": dict(n=200, ranks=[1, 2, 40, 5], fanouts=[1, 7, 20, 32], asz=32, rounds=24, p=0.05,
              prunes=[0, 1179, 3792, 6139]),
    "D": dict(n=150, ranks=[1, 4, 9], fanouts=[1, 3, 7], asz=7, rounds=30, p=0.05, prunes=[0, 297, 882]),
    "E": dict(n=120, ranks=list(range(1, 37)), fanouts=[1 + k % 12 for k in range(36)], asz=12, rounds=26, p=0.05,
              min_prunes=122),
}
FULL_EVERY = 5  # caches, active-set entries and mst every few rounds (and in the last)


@functools.lru_cache(maxsize=None)
def trace(name):
    """The oracle's state after every step of every round of a case, one sim per slot."""
    c = CASES[name]
    n, asz, rounds = c["n"], c["asz"], c["rounds"]
    pks, st = eb.synth.network(n)
    sims = [ob.Sim(ob.PHILOX, SEED, pks, st, f) for f in c["fanouts"]]
    origins = [sims[0].find_nth_largest(r) for r in c["ranks"]]
    for s in sims:
        s.init_philox(asz)
    out = dict(st=st, pks=pks, origins=origins, rounds=[], entries0=sims[0].entries(asz))
    totals = [0] * len(sims)
    for r in range(rounds):
        full = r % FULL_EVERY == 0 or r == rounds - 1
        rec = dict(full=full, slots=[])
        if c.get("fail_at") == r:
            for s, f in zip(sims, c["fractions"]):
                s.fail_nodes(f)
            rec["failed"] = [s.failed() for s in sims]
        for k, (s, o) in enumerate(zip(sims, origins)):
            q = {}
            s.run_gossip(o)
            q["dist"] = s.distances()
            q["orders"] = s.orders_all(64 * n)
            if full:
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
            s.chance_to_rotate(asz, c["p"], r)
            if full:
                q["pruned_rot"] = s.pruned_all(o)
            rec["slots"].append(q)
        if full:
            rec["entries"] = sims[0].entries(asz)
        out["rounds"].append(rec)
    # no case passes on an idle prune path
    for f, t in zip(c["fanouts"], totals):
        assert (t == 0) if f == 1 else (t > 0), (name, c["fanouts"], totals)
    if "prunes" in c:
        assert totals == c["prunes"], (name, totals)
    if "min_prunes" in c:
        assert min(t for f, t in zip(c["fanouts"], totals) if f >= 2) == c["min_prunes"], (name, totals)
    out["totals"] = totals
    return out


def make_engine(name, **kw):
    c, t = CASES[name], trace(name)
    eng = gs.Engine(t["st"], len(c["ranks"]), fanout=max(c["fanouts"]), active_set_size=c["asz"],
                    rotation_probability=c["p"], seed=SEED, **kw)
    eng.set_slots(t["origins"], MI, THR)
    eng.set_slot_fanouts(c["fanouts"])
    eng.init_active_sets()
    return eng


def assert_entries(eng, want):
    gp, gl = eng.active_sets()
    op, ol = want
    np.testing.assert_array_equal(gl, ol)
    np.testing.assert_array_equal(np.where(gp == 0xFFFFFFFF, 0, gp), np.where(op == 0xFFFFFFFF, 0, op))


def assert_caches(eng, k, want, msg):
    up, ln, keys, sc = eng.caches(k)
    oup, oln, okeys, osc = want
    has = oup != 0xFFFFFFFF
    np.testing.assert_array_equal(up[has], oup[has], err_msg=msg)
    np.testing.assert_array_equal(up[~has], 0, err_msg=msg)
    np.testing.assert_array_equal(ln, oln, err_msg=msg)
    np.testing.assert_array_equal(keys, okeys, err_msg=msg)
    np.testing.assert_array_equal(sc, osc, err_msg=msg)


def run_steps(name, **kw):
    """The step-wise round of the engine against the case's trace."""
    c, t = CASES[name], trace(name)
    n, S = c["n"], len(c["ranks"])
    eng = make_engine(name, **kw)
    assert_entries(eng, t["entries0"])
    for r, rec in enumerate(t["rounds"]):
        if "failed" in rec:
            eng.fail_nodes(c["fractions"])
            for k in range(S):
                np.testing.assert_array_equal(eng.failed(k), rec["failed"][k])
        eng.run_gossip()
        for k, q in enumerate(rec["slots"]):
            msg = f"{name} slot {k} (fanout {c['fanouts'][k]}) round {r}"
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
                assert_caches(eng, k, q["caches"], "caches " + msg)
        eng.prune_connections()
        for k, q in enumerate(rec["slots"]):
            for got, want in zip(eng.counters(k), q["counters"]):
                np.testing.assert_array_equal(got, want, err_msg=f"counters {name} slot {k} round {r}")
            np.testing.assert_array_equal(eng.pruned_all(k), q["pruned"], err_msg=f"prune state {name} {k} round {r}")
        eng.chance_to_rotate(r)
        if rec["full"]:
            assert_entries(eng, rec["entries"])
            for k, q in enumerate(rec["slots"]):
                np.testing.assert_array_equal(eng.pruned_all(k), q["pruned_rot"])
    return eng


A_STRATEGIES = {
    "workgroup": (dict(bfs_mode=gs.GS_BFS_WORKGROUP), None),
    "level": (dict(bfs_mode=gs.GS_BFS_LEVEL), None),
    "binned": (dict(bfs_mode=gs.GS_BFS_BINNED, binned_all_levels=True), None),
    "multi": (dict(bfs_mode=gs.GS_BFS_MULTI), None),                                # the persistent kernel
    "multi-launched": (dict(bfs_mode=gs.GS_BFS_MULTI), "0"),                         # the launched level loop
    "multi-launched-grid": (dict(bfs_mode=gs.GS_BFS_MULTI, no_small_levels=True), "0"),  # ... every level grid-wide
    "hybrid": (dict(bfs_mode=gs.GS_BFS_HYBRID), None),
}


@pytest.mark.parametrize("strategy", list(A_STRATEGIES))
def test_case_a_every_strategy(strategy, monkeypatch):
    kw, pbfs = A_STRATEGIES[strategy]
    if pbfs is not None:
        monkeypatch.setenv("GS_MV_PBFS", pbfs)  # (read when the engine is created)
    eng = run_steps("A", **kw)
    if strategy == "multi":
        assert eng.info()["bfs_persistent"]
    if strategy.startswith("multi-launched"):
        assert not eng.info()["bfs_persistent"]


@pytest.mark.parametrize("mode", ["level", "binned", "multi"])
def test_case_b_failures(mode):
    """Failed peers burn a slot of each sim's own fanout (gossip.rs:538-541)."""
    run_steps("B", **A_STRATEGIES[mode][0])


@pytest.mark.parametrize("mode", ["binned", "multi"])
def test_case_c_u64_ring(mode):
    """Active-set size 32: the u64 ring selection; the multi BFS has no shared-prefix path."""
    run_steps("C", **A_STRATEGIES[mode][0])


def test_case_d_workgroup():
    run_steps("D", bfs_mode=gs.GS_BFS_WORKGROUP)


@pytest.mark.parametrize("pbfs", ["1", "0"])
def test_case_e_two_slot_groups(pbfs, monkeypatch):
    monkeypatch.setenv("GS_MV_PBFS", pbfs)
    eng = run_steps("E", bfs_mode=gs.GS_BFS_MULTI)
    assert eng.bfs_geometry()["groups"] >= 2
    assert eng.info()["bfs_persistent"] == (pbfs == "1")


# ------------------------------------------------------- one-kernel round ----
@pytest.mark.parametrize("name,fp6", [("A", False), ("D", False), ("A6", True)])
def test_fused_round(name, fp6):
    """gs_round's one-kernel workgroup round: capacity 12 (A) and 7 (D) select the ring
    variant of the kernel, capacity 6 (A6) the compacted-push one."""
    c, t = CASES[name], trace(name)
    assert (max(c["fanouts"]) <= 6) == fp6
    eng = make_engine(name, bfs_mode=gs.GS_BFS_WORKGROUP)
    assert eng.info()["fused_round"]
    S, rounds = len(c["ranks"]), c["rounds"]
    for r, rec in enumerate(t["rounds"]):
        eng.round(r, record=True)
        for k, q in enumerate(rec["slots"]):
            msg = f"{name} slot {k} round {r}"
            np.testing.assert_array_equal(eng.distances(k), q["dist"], err_msg="hops " + msg)
            assert eng.prunes(k) == q["prunes"], "prunes " + msg
            for got, want in zip(eng.counters(k), q["counters"]):
                np.testing.assert_array_equal(got, want, err_msg="counters " + msg)
            if rec["full"]:
                assert_caches(eng, k, q["caches"], "caches " + msg)
                np.testing.assert_array_equal(eng.pruned_all(k), q["pruned_rot"], err_msg="prune state " + msg)
        if rec["full"]:
            summ = eng.summaries()
            assert summ.shape == (r + 1, S)
            for rr in range(r + 1):
                for k, q in enumerate(t["rounds"][rr]["slots"]):
                    assert int(summ[rr, k]["visited"]) == int((q["dist"] != U64MAX).sum())
                    assert int(summ[rr, k]["pushes"]) == len(q["orders"][1])
                    assert int(summ[rr, k]["prunes"]) == len(q["prunes"])


# ------------------------------------------------- engine-level properties ----
def _readbacks(eng, S):
    out = [eng.summaries()]
    for k in range(S):
        out += [eng.hops(k), eng.pruned_all(k), *eng.caches(k), *eng.accumulators(k)]
    return out


@pytest.mark.parametrize("mode", [gs.GS_BFS_WORKGROUP, gs.GS_BFS_MULTI])
def test_uniform_and_null_equal_an_engine_never_called(mode):
    """A uniform array equal to params.push_fanout, and NULL after a non-uniform array, leave
    an engine identical to one that never received the call."""
    _, st = eb.synth.network(240)
    origins, S = [3, 77, 150, 239], 4
    engines = [gs.Engine(st, S, fanout=6, active_set_size=12, rotation_probability=0.05, seed=SEED, bfs_mode=mode)
               for _ in range(3)]
    for e in engines:
        e.set_slots(origins, MI, THR)
    engines[1].set_slot_fanouts([6] * S)
    engines[2].set_slot_fanouts([1, 2, 3, 6])
    engines[2].set_slot_fanouts(None)
    for e in engines:
        np.testing.assert_array_equal(e.slot_fanouts(), [6] * S)
        e.init_active_sets()
        for r in range(12):
            e.round(r, record=True)
    want = _readbacks(engines[0], S)
    assert (want[1] != 0xFF).sum() > 1
    for e in engines[1:]:
        for a, b in zip(_readbacks(e, S), want):
            np.testing.assert_array_equal(a, b)


def test_get_round_trips_and_bad_values_are_refused():
    _, st = eb.synth.network(100)
    eng = gs.Engine(st, 3, fanout=5, active_set_size=12, seed=SEED, bfs_mode=gs.GS_BFS_LEVEL)
    np.testing.assert_array_equal(eng.slot_fanouts(), [5, 5, 5])
    eng.set_slots([1, 2, 3])
    eng.set_slot_fanouts([1, 5, 3])
    np.testing.assert_array_equal(eng.slot_fanouts(), [1, 5, 3])
    for bad in ([0, 5, 3], [1, 6, 3]):
        with pytest.raises(gs.GsError) as ei:
            eng.set_slot_fanouts(bad)
        assert ei.value.code == -1 and "slot " + str(bad.index(0) if 0 in bad else 1) in str(ei.value)
        np.testing.assert_array_equal(eng.slot_fanouts(), [1, 5, 3])  # unchanged
    eng.init_active_sets()  # still usable
    eng.run_gossip()
    eg = [int(eng.counters(k)[0].max()) for k in range(3)]
    assert eg == [1, 5, 3]  # egress of a node = its slot's fanout at most, reached by some node
    eng.set_slot_fanouts(None)
    np.testing.assert_array_equal(eng.slot_fanouts(), [5, 5, 5])


# ------------------------------------------------------------- whole sims ----
F64_NAMES = ["coverage", "rmr", "branching", "hop_mean", "hop_median", "coverage_stats", "rmr_stats",
             "branching_stats", "aggregate_hops", "ldh", "stranded", "stranded_round_mean", "stranded_round_median"]
U64_NAMES = ["origin", "hop_max", "hop_min", "aggregate_hops", "ldh", "stranded", "stranded_times",
             "stranded_round_count", "stranded_round_max", "stranded_round_min", "hops_hist", "stranded_hist",
             "egress_hist", "ingress_hist", "prune_hist", "egress_cpb", "validator_hist", "hist_errors",
             "failed_count"]


def test_run_simulations_with_fanouts():
    pks, st = eb.synth.network(220)
    fanouts = [2, 6, 11]
    res = gs.run_simulations(st, n_sims=3, origin_ranks=[1, 1, 1], iterations=45, warm_up=5, seed=9,
                             fanouts=fanouts)
    for k, f in enumerate(fanouts):
        o = ob.run_simulation(pks, st, origin_rank=1, iterations=45, warm_up=5, seed=9, fanout=f)
        for name in F64_NAMES:
            np.testing.assert_array_equal(res.f64(k, name), o.f64(name), err_msg=f"sim {k} {name}")
        for name in U64_NAMES:
            np.testing.assert_array_equal(res.u64(k, name), o.u64(name), err_msg=f"sim {k} {name}")


def test_run_fanout_sweep_equals_run_sweep():
    """sweep.run_fanout_sweep (one engine per active-set size) == run_sweep (one per value)."""
    import gossip_sim_amd.sweep as sw
    _, st = eb.synth.network(150)
    fanouts = [2, 5, 13]

    def cfg(f):
        return dict(fanout=f, asz=max(12, f), iterations=30, warm_up=5, seed=4)

    a = sw.run_fanout_sweep(st, fanouts, lambda f: dict(cfg(f), asz=12))
    b = sw.run_sweep(st, fanouts, cfg)
    for i in range(3):
        for kind, name in sw.NAMES:
            np.testing.assert_array_equal(a.per_sim[i][(kind, name)], b.per_sim[i][(kind, name)], err_msg=name)


# -------------------------------------------------------------- partition ----
def _part_round(eng, L, r, record, frontier, bufs):
    """One round of a one-rank node-range partition through host buffers (no collective)."""
    h, n = eng.h, C.c_uint32()
    if frontier:
        ng = C.c_uint32()
        gs._check(L.gs_part_xbfs_groups(h, C.byref(ng)))
        w = np.zeros(1, dtype=np.uint64)
        for g in range(ng.value):
            gs._check(L.gs_part_xbfs_begin(h, g, C.byref(n)))
            d = 0
            while n.value:
                gs._check(L.gs_part_xbfs_expand(h, d, w.ctypes.data_as(C.c_void_p)))
                msg = np.zeros(max(1, int(w[0])), dtype=np.uint64)
                gs._check(L.gs_part_xbfs_send(h, msg.ctypes.data_as(C.c_void_p), 0))
                gs._check(L.gs_part_xbfs_apply(h, d, msg.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p), 0,
                                               C.byref(n)))
                d += 1
            gs._check(L.gs_part_xbfs_end(h, int(record)))
        gs._check(L.gs_part_xround_finish(h, r, int(record), C.byref(n)))
    else:
        gs._check(L.gs_part_round(h, r, int(record), C.byref(n)))
    if n.value:
        gs._check(L.gs_part_prunes_dense_out(h, bufs["dense"].ctypes.data_as(C.c_void_p), 0))
        gs._check(L.gs_part_prunes_dense_in(h, bufs["dense"].ctypes.data_as(C.c_void_p), 0))
    eng.chance_to_rotate(r)
    if record:
        gs._check(L.gs_part_stats_out(h, bufs["stats"].ctypes.data_as(C.c_void_p), 0))
        gs._check(L.gs_part_stats_in(h, bufs["stats"].ctypes.data_as(C.c_void_p), 0))


@pytest.mark.parametrize("frontier", [False, True])
def test_partition_rank_takes_slot_fanouts(frontier):
    """A one-rank gs_create_part engine (replicated BFS and frontier exchange) with per-slot
    fanouts equals a plain MULTI engine given the same fanouts: the "small" case of
    tests/partition_case.py, every array test_partition.py compares for it."""
    import partition_case as pc
    c = pc.CASES["small"]
    st = pc.stakes_of("small", eb.synth)
    S, fanouts = len(c["mi"]), [2, 6, 9]
    L = gs.lib()

    class Part:  # run_case drives an engine through round(); the rest is the Engine's
        def __init__(self):
            self.eng = gs.Engine(st, S, fanout=9, seed=c["seed"], rotation_probability=c["p"],
                                 bfs_mode=gs.GS_BFS_MULTI, part=(0, 1), frontier_exchange=frontier)
            sw, lo, hi = C.c_size_t(), C.c_uint32(), C.c_uint32()
            gs._check(L.gs_part_sizes(self.eng.h, C.byref(sw), C.byref(lo), C.byref(hi)))
            assert (lo.value, hi.value) == (0, c["n"])
            rc, dw = C.c_size_t(), C.c_size_t()
            gs._check(L.gs_part_exchange_sizes(self.eng.h, C.byref(rc), C.byref(dw)))
            self.bufs = dict(stats=np.zeros(sw.value, dtype=np.uint64), dense=np.zeros(dw.value, dtype=np.uint32))

        def __getattr__(self, name):
            return getattr(self.eng, name)

        def set_slots(self, *a):
            self.eng.set_slots(*a)
            self.eng.set_slot_fanouts(fanouts)

        def round(self, r, record=False):
            _part_round(self.eng, L, r, record, frontier, self.bufs)

    class Plain(Part):
        def __init__(self):
            self.eng = gs.Engine(st, S, fanout=9, seed=c["seed"], rotation_probability=c["p"],
                                 bfs_mode=gs.GS_BFS_MULTI)

        def round(self, r, record=False):
            self.eng.round(r, record=record)

    got = pc.run_case(Part(), "small", st)
    want = pc.run_case(Plain(), "small", st)
    assert want["summaries"]["prunes"].sum() > 0
    pushes = want["summaries"]["pushes"].sum(axis=0)
    assert pushes[0] < pushes[1] < pushes[2]  # the slots' fanouts took effect
    assert sorted(got) == sorted(want)
    for key in want:
        np.testing.assert_array_equal(got[key], want[key], err_msg=key)


# -------------------------------------------------------------------- CLI ----
from test_cli import F64_NAMES as CLI_F64, U64_NAMES as CLI_U64, cli, oracle_sims, sweep_params, yaml_net  # noqa: E402,F401
import report_ref as rr  # noqa: E402


def test_cli_push_fanout_sweep_batches(yaml_net, tmp_path):
    """--test-type push-fanout with fanouts 2, 5, 8, 11, 14 of active-set size 12: two engines
    (four sims at size 12, one at 14), results equal to the oracle's per sim."""
    path, keys, st, pks = yaml_net
    iters, warm, seed = 34, 6, 13
    params = sweep_params(3, 5, iterations=iters, warm_up=warm, step=3, fanout=2)
    assert [p["fanout"] for p in params] == [2, 5, 8, 11, 14] and [p["asz"] for p in params] == [12] * 4 + [14]
    res, plan = str(tmp_path / "g.txt"), str(tmp_path / "plan.txt")
    r = cli("--accounts-from-yaml", "--account-file", path, "--iterations", iters, "--warm-up-rounds", warm,
            "--test-type", "push-fanout", "--push-fanout", 2, "--step-size", 3, "--num-simulations", 5,
            "--origin-rank", 1, 1, 1, 1, 1, 1, "--print-stats", "--save-results", res, "--seed", seed,
            "--engine-plan", plan)
    assert open(plan).read().splitlines() == ["device 0 sims 0,1,2,3 active-set-size 12 fanouts 2,5,8,11",
                                              "device 0 sims 4 active-set-size 14 fanouts 14"]
    got = rr.read_results(res)
    want = oracle_sims(pks, st, params, seed=seed)
    for k, ((gf, gu), (wf, wu)) in enumerate(zip(got, want)):
        for n in CLI_F64:
            np.testing.assert_array_equal(gf[n], wf[n], err_msg=f"sim {k} {n}")
        for n in CLI_U64:
            np.testing.assert_array_equal(gu[n], wu[n], err_msg=f"sim {k} {n}")
    assert rr.report_lines(r.stderr) == rr.render(keys, st, want, params, iterations=iters, warm_up=warm,
                                                  num_sims=5, test_type=3)
