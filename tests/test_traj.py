"""Active-set trajectory tables (gs_create_traj): one engine holding several PushActiveSet
tables, each with its own active-set size and rotation probability and serving a contiguous
range of slots. Slot k is compared, bit for bit and round by round, with an oracle sim built
with the slot's own fanout and its table's size and probability -- in the one-kernel round,
the step-wise round, the split round, the stand-alone rotation, whole sims, the batched sweep
and the CLI's --batch-sweeps.

Each case's oracle trace is computed once and shared by the tests that run it. The cases
(synth.network, seed 7, threshold 0.15, min-ingress 2; a slot is (table, origin rank, fanout))
and the prunes each slot emits over the case's rounds in the oracle alone, asserted in the
trace so that no case passes on an idle prune path:
  A  240 nodes, sizes 6 / 12 / 20 (u32 push masks, the 6-push compacted kernel):
     1309, 1304, 1315, 1329, 1313, 1327
  B  200 nodes, size 12 with p = 0 / .05 / .5 / 1 (the ring kernel): 1981, 2171, 2164, 3795, 5547, 5567
  C  150 nodes, sizes 7 / 12 with per-slot fanouts (the fanout-1 slot prunes nothing):
     0, 297, 882, 168, 1183, 1626
  D  200 nodes, sizes 12 / 32 (capacity 32): 987, 2172, 987, 3792, 6139
  E  180 nodes, sizes 4 / 16 (u16 masks), fail-nodes at round 2: 384, 72, 539, 1274
"""
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
    "A": dict(n=240, rounds=30, tables=[(6, .08), (12, .08), (20, .08)],
              slots=[(0, 1, 6), (0, 7, 6), (1, 1, 6), (1, 60, 6), (2, 1, 6), (2, 240, 6)],
              prunes=[1309, 1304, 1315, 1329, 1313, 1327]),
    "B": dict(n=200, rounds=30, tables=[(12, 0.), (12, .05), (12, .5), (12, 1.)],
              slots=[(0, 1, 12), (1, 1, 12), (1, 5, 12), (2, 1, 12), (3, 1, 12), (3, 40, 12)],
              prunes=[1981, 2171, 2164, 3795, 5547, 5567]),
    "C": dict(n=150, rounds=30, tables=[(7, .05), (12, .05)],
              slots=[(0, 1, 1), (0, 4, 3), (0, 9, 7), (1, 1, 2), (1, 4, 9), (1, 9, 12)],
              prunes=[0, 297, 882, 168, 1183, 1626]),
    "D": dict(n=200, rounds=24, tables=[(12, .05), (32, .05)],
              slots=[(0, 1, 6), (0, 2, 12), (1, 1, 6), (1, 40, 20), (1, 5, 32)],
              prunes=[987, 2172, 987, 3792, 6139]),
    "E": dict(n=180, rounds=30, tables=[(4, .03), (16, .03)],
              slots=[(0, 1, 4), (0, 3, 2), (1, 5, 6), (1, 9, 16)],
              prunes=[384, 72, 539, 1274], fail_at=2, fractions=[.1, .2, .3, .5]),
}
FULL_EVERY = 5  # caches, active-set entries and mst every few rounds (and in the last)


def trajectories(c):
    """The engine's tables (size, probability, slots): the case's slots are grouped by table."""
    tabs = [t for t, _, _ in c["slots"]]
    assert tabs == sorted(tabs)
    return [(a, p, tabs.count(t)) for t, (a, p) in enumerate(c["tables"])]


@functools.lru_cache(maxsize=None)
def trace(name):
    """The oracle's state after every step of every round of a case: one sim per slot, built
    with the slot's own fanout and run with its table's size and probability."""
    c = CASES[name]
    n, rounds = c["n"], c["rounds"]
    pks, st = eb.synth.network(n)
    sims = [ob.Sim(ob.PHILOX, SEED, pks, st, f) for _, _, f in c["slots"]]
    origins = [sims[0].find_nth_largest(r) for _, r, _ in c["slots"]]
    size = [c["tables"][t][0] for t, _, _ in c["slots"]]
    prob = [c["tables"][t][1] for t, _, _ in c["slots"]]
    first = [[t for t, _, _ in c["slots"]].index(t) for t in range(len(c["tables"]))]  # a sim of each table
    for s, a in zip(sims, size):
        s.init_philox(a)
    out = dict(st=st, pks=pks, origins=origins, rounds=[],
               entries0=[sims[k].entries(c["tables"][t][0]) for t, k in enumerate(first)])
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
            s.chance_to_rotate(size[k], prob[k], r)
            if full:
                q["pruned_rot"] = s.pruned_all(o)
            rec["slots"].append(q)
        if full:
            rec["entries"] = [sims[k].entries(c["tables"][t][0]) for t, k in enumerate(first)]
        out["rounds"].append(rec)
    assert totals == c["prunes"], (name, totals)  # (no case passes on an idle prune path)
    return out


def make_engine(name, **kw):
    c, t = CASES[name], trace(name)
    fanouts = [f for _, _, f in c["slots"]]
    eng = gs.Engine(t["st"], len(c["slots"]), fanout=max(fanouts), seed=SEED, trajectories=trajectories(c), **kw)
    eng.set_slots(t["origins"], MI, THR)
    if len(set(fanouts)) > 1:
        eng.set_slot_fanouts(fanouts)
    eng.init_active_sets()
    return eng


def assert_entries(eng, want):
    """Every table's entries against the oracle's at that table's own size."""
    for t, (op, ol) in enumerate(want):
        gp, gl = eng.active_sets(table=t)
        assert gp.shape == op.shape, f"table {t}"
        np.testing.assert_array_equal(gl, ol, err_msg=f"table {t}")
        np.testing.assert_array_equal(np.where(gp == 0xFFFFFFFF, 0, gp), np.where(op == 0xFFFFFFFF, 0, op),
                                      err_msg=f"table {t}")


def assert_caches(eng, k, want, msg):
    up, ln, keys, sc = eng.caches(k)
    oup, oln, okeys, osc = want
    has = oup != 0xFFFFFFFF
    np.testing.assert_array_equal(up[has], oup[has], err_msg=msg)
    np.testing.assert_array_equal(up[~has], 0, err_msg=msg)
    np.testing.assert_array_equal(ln, oln, err_msg=msg)
    np.testing.assert_array_equal(keys, okeys, err_msg=msg)
    np.testing.assert_array_equal(sc, osc, err_msg=msg)


def run_rounds(name, **kw):
    """gs_round (the one-kernel round, or with split_round the step kernels) against the trace."""
    c, t = CASES[name], trace(name)
    eng = make_engine(name, **kw)
    S = len(c["slots"])
    assert_entries(eng, t["entries0"])
    for r, rec in enumerate(t["rounds"]):
        if "failed" in rec:
            eng.fail_nodes(c["fractions"])
            for k in range(S):
                np.testing.assert_array_equal(eng.failed(k), rec["failed"][k])
        eng.round(r, record=True)
        for k, q in enumerate(rec["slots"]):
            msg = f"{name} slot {k} {c['slots'][k]} round {r}"
            np.testing.assert_array_equal(eng.distances(k), q["dist"], err_msg="hops " + msg)
            assert eng.prunes(k) == q["prunes"], "prunes " + msg
            for got, want in zip(eng.counters(k), q["counters"]):
                np.testing.assert_array_equal(got, want, err_msg="counters " + msg)
            if rec["full"]:
                assert_caches(eng, k, q["caches"], "caches " + msg)
                np.testing.assert_array_equal(eng.pruned_all(k), q["pruned_rot"], err_msg="prune state " + msg)
        if rec["full"]:
            assert_entries(eng, rec["entries"])
            summ = eng.summaries()
            assert summ.shape == (r + 1, S)
            for rr in range(r + 1):
                for k, q in enumerate(t["rounds"][rr]["slots"]):
                    assert int(summ[rr, k]["visited"]) == int((q["dist"] != U64MAX).sum())
                    assert int(summ[rr, k]["pushes"]) == len(q["orders"][1])
                    assert int(summ[rr, k]["prunes"]) == len(q["prunes"])
    return eng


@pytest.mark.parametrize("name", list(CASES))
def test_fused_round(name):
    eng = run_rounds(name)
    assert eng.info()["fused_round"] and eng.info()["bfs_mode"] == gs.GS_BFS_WORKGROUP


def test_case_b_split_round():
    eng = run_rounds("B", split_round=True)
    assert not eng.info()["fused_round"]


def test_case_b_standalone_rotation(monkeypatch):
    """GS_ROT_AHEAD=0: the rotation launches of every table and the round kernel's deferred clear."""
    monkeypatch.setenv("GS_ROT_AHEAD", "0")  # (read when the engine is created)
    eng = run_rounds("B")
    assert eng.info()["fused_round"]


@pytest.mark.parametrize("name", ["A", "C"])
def test_stepwise_round(name):
    """run_gossip ... chance_to_rotate, with the inbound lists and mst of every slot."""
    c, t = CASES[name], trace(name)
    n, S = c["n"], len(c["slots"])
    eng = make_engine(name)
    assert_entries(eng, t["entries0"])
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


# ------------------------------------------------- engine-level properties ----
def _readbacks(eng, S):
    out = [eng.summaries()]
    for k in range(S):
        out += [eng.hops(k), eng.pruned_all(k), *eng.caches(k), *eng.accumulators(k)]
    return out


def test_one_table_equals_a_plain_engine():
    _, st = eb.synth.network(240)
    origins, S = [3, 77, 150, 239], 4
    a = gs.Engine(st, S, fanout=6, seed=SEED, trajectories=[(12, .05, S)])
    b = gs.Engine(st, S, fanout=6, seed=SEED, active_set_size=12, rotation_probability=.05,
                  bfs_mode=gs.GS_BFS_WORKGROUP)
    assert a.trajectories() == b.trajectories() == [(12, .05, S)]
    assert a.info() == b.info()
    for e in (a, b):
        e.set_slots(origins, MI, THR)
        e.init_active_sets()
        for r in range(12):
            e.round(r, record=True)
    want = _readbacks(b, S)
    assert (want[1] != 0xFF).sum() > 1
    for x, y in zip(_readbacks(a, S), want):
        np.testing.assert_array_equal(x, y)
    for x, y in zip(a.active_sets(), b.active_sets()):  # (the un-suffixed call: one table)
        np.testing.assert_array_equal(x, y)


def test_tables_equal_single_table_engines_at_3000_nodes():
    """The workload's node count, kept short: every slot of a three-table engine against the
    single-table engine created with its table's values. 24 rounds, not fewer: a cache entry
    prunes at its 20th upsert (one per round at most), so no prune exists before round 20 and
    the summed prunes asserted below would be 0."""
    _, st = eb.synth.network(3000)
    tabs, per, rounds = [(12, .01), (20, .01), (27, .01)], 2, 24
    origins = [5, 1700] * len(tabs)

    def run(eng, org):
        eng.set_slots(org, MI, THR)
        eng.init_active_sets()
        for r in range(rounds):
            eng.round(r, record=True)
        return eng

    multi = run(gs.Engine(st, per * len(tabs), fanout=6, seed=SEED, trajectories=[(a, p, per) for a, p in tabs]), origins)
    assert multi.info()["fused_round"]
    ms = multi.summaries()
    total = 0
    for t, (a, p) in enumerate(tabs):
        one = run(gs.Engine(st, per, fanout=6, seed=SEED, active_set_size=a, rotation_probability=p,
                            bfs_mode=gs.GS_BFS_WORKGROUP), origins[:per])
        os_ = one.summaries()
        for j in range(per):
            k = t * per + j
            np.testing.assert_array_equal(multi.hops(k), one.hops(j), err_msg=f"hops table {t} slot {j}")
            np.testing.assert_array_equal(multi.pruned_all(k), one.pruned_all(j), err_msg=f"pruned table {t} slot {j}")
            for x, y in zip(multi.caches(k), one.caches(j)):
                np.testing.assert_array_equal(x, y, err_msg=f"caches table {t} slot {j}")
            np.testing.assert_array_equal(ms[:, k], os_[:, j], err_msg=f"summaries table {t} slot {j}")
        for x, y in zip(multi.active_sets(table=t), one.active_sets()):
            np.testing.assert_array_equal(x, y, err_msg=f"entries table {t}")
        total += int(os_["prunes"].sum())
    assert total > 0


def test_refusals_and_round_trip():
    _, st = eb.synth.network(100)

    def make(tr, n_slots=3, st=st, **kw):
        return gs.Engine(st, n_slots, fanout=6, active_set_size=12, seed=SEED, trajectories=tr, **kw)

    bad = [[],                                  # n_traj == 0
           [(12, .1, 3), (8, .1, 0)],           # a table without slots
           [(0, .1, 1), (12, .1, 2)],           # size 0
           [(33, .1, 1), (12, .1, 2)],          # size above GS_MAX_ACTIVE_SET_SIZE (and so above any capacity)
           [(12, -.1, 1), (12, .1, 2)],         # probability outside [0, 1]
           [(12, 1.5, 1), (12, .1, 2)],
           [(12, float("nan"), 1), (12, .1, 2)],
           [(12, .1, 1), (8, .1, 1)],           # counts do not sum to n_slots
           [(12, .1, 2), (8, .1, 2)]]
    for tr in bad:
        with pytest.raises(gs.GsError) as ei:
            make(tr)
        assert ei.value.code == -1, tr
    # a size above the capacity, through the C ABI (the Python class sizes the capacity itself)
    import ctypes as C
    p = gs.Params(6, 8, 0., SEED, 0, gs.GS_BFS_AUTO, 0, 0)
    arr = (gs.Traj * 2)(gs.Traj(8, .1, 1), gs.Traj(9, .1, 2))
    h = C.c_void_p()
    stc = np.ascontiguousarray(st, dtype=np.uint64)
    assert gs.lib().gs_create_traj(C.byref(p), stc.ctypes.data_as(C.c_void_p), len(stc), 3, C.cast(arr, C.c_void_p), 2,
                                   C.byref(h)) == -1
    assert not h.value and b"params.active_set_size" in gs.lib().gs_last_error()
    for mode in (gs.GS_BFS_LEVEL, gs.GS_BFS_BINNED, gs.GS_BFS_MULTI, gs.GS_BFS_HYBRID):
        with pytest.raises(gs.GsError) as ei:
            make([(12, .1, 1), (8, .1, 2)], bfs_mode=mode)
        assert ei.value.code == -1 and "GS_BFS_WORKGROUP" in str(ei.value)
    # a node count the workgroup engine's LDS cannot hold
    big = 70000
    assert gs.traj_supported(big, 6, 12) == (False, False)
    with pytest.raises(gs.GsError) as ei:
        make([(12, .1, 1), (8, .1, 2)], st=np.full(big, 10**9, dtype=np.uint64))
    assert ei.value.code == -1 and "LDS" in str(ei.value)
    # a valid create afterwards still works; AUTO resolves to WORKGROUP at any slot count
    tr = [(12, .25, 1), (8, .5, 2)]
    eng = make(tr)
    assert eng.trajectories() == tr
    assert eng.info()["bfs_mode"] == gs.GS_BFS_WORKGROUP and eng.info()["fused_round"]
    eng.set_slots([1, 2, 3], MI, THR)
    eng.init_active_sets()
    for call in (eng.active_sets, lambda: eng.get_entry(3, 0), lambda: eng.set_entry(3, 0, [1, 2])):
        with pytest.raises(gs.GsError) as ei:
            call()
        assert ei.value.code == -1 and "_traj" in str(ei.value)
    with pytest.raises(gs.GsError):
        eng.active_sets(table=2)
    assert eng.active_sets(table=1)[0].shape == (100, 25, 8)
    # an uploaded entry reads back, and clears the prune state of its own table's slots only
    for r in range(25):
        eng.round(r)
    before = [eng.pruned_all(k) for k in range(3)]
    node = int(np.argmax(before[1] | before[2]))
    assert (before[1] | before[2])[node] and before[0].any()
    bucket = eng.get_entry(node, 0, table=1)
    for b in range(25):
        eng.set_entry(node, b, [(node + 1) % 100, (node + 2) % 100], table=1)
    assert eng.get_entry(node, 3, table=1) == [(node + 1) % 100, (node + 2) % 100]
    assert len(bucket) <= 8
    after = [eng.pruned_all(k) for k in range(3)]
    np.testing.assert_array_equal(after[0], before[0])
    assert after[1][node] == 0 and after[2][node] == 0
    eng.round(25)
    eng.sync()


# ------------------------------------------------------------- whole sims ----
from test_slot_fanout import F64_NAMES, U64_NAMES  # noqa: E402


def test_run_simulations_with_tables():
    """Equal (size, probability) pairs need not be adjacent; results come back in sim order."""
    pks, st = eb.synth.network(220)
    aszs, probs, fanouts = [8, 12, 12, 20], [.02, .02, .3, .02], [3, 6, 6, 9]
    res = gs.run_simulations(st, n_sims=4, aszs=aszs, rot_probs=probs, fanouts=fanouts, iterations=45, warm_up=5,
                             seed=9)
    for k, (a, p, f) in enumerate(zip(aszs, probs, fanouts)):
        o = ob.run_simulation(pks, st, origin_rank=1, iterations=45, warm_up=5, seed=9, asz=a, p=p, fanout=f)
        for name in F64_NAMES:
            np.testing.assert_array_equal(res.f64(k, name), o.f64(name), err_msg=f"sim {k} {name}")
        for name in U64_NAMES:
            np.testing.assert_array_equal(res.u64(k, name), o.u64(name), err_msg=f"sim {k} {name}")
    # the same pairs interleaved: sims 0 and 2 share a table, as do 1 and 3
    res = gs.run_simulations(st, n_sims=4, aszs=[8, 12, 8, 12], rot_probs=[.02] * 4, origin_ranks=[1, 1, 2, 2],
                             iterations=30, warm_up=5, seed=9)
    for k, (a, rk) in enumerate(zip([8, 12, 8, 12], [1, 1, 2, 2])):
        o = ob.run_simulation(pks, st, origin_rank=rk, iterations=30, warm_up=5, seed=9, asz=a, p=.02)
        for name in F64_NAMES:
            np.testing.assert_array_equal(res.f64(k, name), o.f64(name), err_msg=f"sim {k} {name}")
        for name in U64_NAMES:
            np.testing.assert_array_equal(res.u64(k, name), o.u64(name), err_msg=f"sim {k} {name}")


def test_run_traj_sweep_equals_run_sweep():
    import gossip_sim_amd.sweep as sw
    _, st = eb.synth.network(150)
    sizes = [6, 12, 18]
    calls = []

    def runner(stakes, **kw):
        calls.append(kw["n_sims"])
        return gs.run_simulations(stakes, **kw)

    def cfg(a):
        return dict(asz=a, iterations=30, warm_up=5, seed=4)

    a = sw.run_traj_sweep(st, sizes, cfg, runner=runner)
    assert calls == [3]  # one engine
    b = sw.run_sweep(st, sizes, cfg)
    for i in range(3):
        for kind, name in sw.NAMES:
            np.testing.assert_array_equal(a.per_sim[i][(kind, name)], b.per_sim[i][(kind, name)], err_msg=name)


# -------------------------------------------------------------------- CLI ----
from test_cli import F64_NAMES as CLI_F64, U64_NAMES as CLI_U64, cli, oracle_sims, sweep_params, yaml_net  # noqa: E402,F401
import report_ref as rr  # noqa: E402


@pytest.mark.parametrize("kind", ["active-set-size", "rotate-probability"])
def test_cli_batch_sweeps(kind, yaml_net, tmp_path):
    """--batch-sweeps: the three sims of an engine-changing sweep as one engine of three tables;
    results equal to the oracle's per sim, the report unchanged, the plan one line of lists."""
    path, keys, st, pks = yaml_net
    iters, warm, seed = 34, 6, 13
    test_type, step = (1, 2) if kind == "active-set-size" else (7, 0.25)
    params = sweep_params(test_type, 3, iterations=iters, warm_up=warm, step=step)
    res, plan = str(tmp_path / "g.txt"), str(tmp_path / "plan.txt")
    r = cli("--accounts-from-yaml", "--account-file", path, "--iterations", iters, "--warm-up-rounds", warm,
            "--test-type", kind, "--step-size", step, "--num-simulations", 3, "--origin-rank", 1, 1, 1, 1,
            "--print-stats", "--save-results", res, "--seed", seed, "--engine-plan", plan, "--batch-sweeps")
    assert open(plan).read().splitlines() == [
        "device 0 sims 0,1,2 active-set-size " + ",".join(str(p["asz"]) for p in params) + " fanouts 6,6,6" +
        " rotation-probability " + ",".join("%.17g" % p["p"] for p in params)]
    assert len({(p["asz"], p["p"]) for p in params}) == 3
    got = rr.read_results(res)
    want = oracle_sims(pks, st, params, seed=seed)
    for k, ((gf, gu), (wf, wu)) in enumerate(zip(got, want)):
        for n in CLI_F64:
            np.testing.assert_array_equal(gf[n], wf[n], err_msg=f"sim {k} {n}")
        for n in CLI_U64:
            np.testing.assert_array_equal(gu[n], wu[n], err_msg=f"sim {k} {n}")
    assert rr.report_lines(r.stderr) == rr.render(keys, st, want, params, iterations=iters, warm_up=warm,
                                                  num_sims=3, test_type=test_type)
