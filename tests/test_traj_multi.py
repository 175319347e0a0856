"""Trajectory tables on the multi-source BFS (gs_create_traj with GS_FLAG_TRAJ_MULTI, bfs_mode
GS_BFS_MULTI): one engine holding several PushActiveSet tables at any node count the multi BFS
supports. Slot groups stay consecutive runs of slots and a frontier entry belongs to one table.

1. test_traj's cases A-E (their oracle traces and pinned prune totals) through the multi table
   engine: the persistent kernel, the launched level loop (GS_MV_PBFS=0), every level through
   expand / apply (no_small_levels) and the narrow consume paths.
2. Case F: 260 nodes, 32 slots in four tables of eight, so the slot groups are 28 + 4 and table 3
   (slots 24..31) straddles the boundary; origins across stake buckets, one origin repeated
   inside a table (slots 0, 1), origins in two tables (slots 0 and 8, slots 9 and 24). 24
   rounds, not 16: a cache entry prunes at its 20th upsert (one per round at most), so the
   oracle alone emits its first prune in round 19 (counting from 0) and 16 rounds gave a total
   of 0 in every slot. The totals below are the oracle's alone, computed on the CPU.
3. Case G: 400 nodes, 28 one-slot tables (sizes 6..32, then 6), nothing shared inside the group,
   against the workgroup table engine (oracle-pinned by test_traj.py).
4. 20,000 nodes -- beyond the workgroup engine -- against single-table GS_BFS_MULTI engines.
5. Refusals, AUTO, the round trip of an uploaded entry.
6. run_simulations, run_traj_sweep and gossip-sim --batch-sweeps --bfs-mode 4.
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
SEED, THR, MI = tt.SEED, tt.THR, tt.MI
MULTI = dict(bfs_mode=gs.GS_BFS_MULTI, traj_multi=True)


def _is_multi(eng):
    info = eng.info()
    return info["bfs_mode"] == gs.GS_BFS_MULTI and not info["fused_round"]


# ------------------------------------------------ 1. the oracle, round by round ----
@pytest.mark.parametrize("name", list(tt.CASES))
def test_oracle_rounds_persistent(name):
    """A: three sizes; B: four probabilities incl. 0 and 1; C: per-slot fanouts; D: capacity 32 (no
    shared-prefix path); E: fail_nodes (failure classes in per-table own rows)."""
    eng = tt.run_rounds(name, **MULTI)
    assert _is_multi(eng) and eng.info()["bfs_persistent"]  # (k_mv_pbfs ran the levels)


@pytest.mark.parametrize("name", ["A", "C", "E"])
def test_oracle_rounds_launched_loop(name, monkeypatch):
    monkeypatch.setenv("GS_MV_PBFS", "0")  # (read when the engine is created)
    eng = tt.run_rounds(name, **MULTI)
    assert _is_multi(eng) and not eng.info()["bfs_persistent"]


@pytest.mark.parametrize("name", ["A", "C", "E"])
def test_oracle_rounds_every_level_through_expand_apply(name, monkeypatch):
    monkeypatch.setenv("GS_MV_PBFS", "0")
    eng = tt.run_rounds(name, no_small_levels=True, **MULTI)
    assert _is_multi(eng) and not eng.info()["bfs_persistent"]


@pytest.mark.parametrize("name", ["A", "C", "E"])
def test_oracle_rounds_narrow_wave_path(name):
    assert _is_multi(tt.run_rounds(name, narrow_wave_path=True, **MULTI))


# ------------------------------------------------ 2. a table straddling a group boundary ----
F = dict(n=260, rounds=24, tables=[(6, .05), (12, .02), (20, .2), (27, .05)],
         ranks=[1, 1, 3, 10, 40, 90, 150, 260,      # table 0 (rank 1 twice)
                1, 2, 5, 20, 60, 120, 200, 250,     # table 1 (rank 1: also in table 0)
                4, 7, 15, 30, 75, 130, 180, 240,    # table 2
                2, 6, 12, 25, 50, 100, 160, 220],   # table 3: slots 24..31, groups 28 + 4
         prunes=[1294, 1294, 1290, 1295, 1298, 1301, 1297, 1297, 1144, 1144, 1136, 1144, 1142, 1145, 1144, 1146,
                 2040, 2050, 2024, 2032, 2038, 2035, 2040, 2028, 1300, 1303, 1302, 1297, 1312, 1296, 1301, 1301])


@functools.lru_cache(maxsize=None)
def f_trace():
    """The oracle alone: one sim per slot at its table's size and probability."""
    n, rounds = F["n"], F["rounds"]
    pks, st = eb.synth.network(n)
    tab = [k // 8 for k in range(32)]
    sims = [ob.Sim(ob.PHILOX, SEED, pks, st, 6) for _ in range(32)]
    origins = [sims[0].find_nth_largest(r) for r in F["ranks"]]
    for s, t in zip(sims, tab):
        s.init_philox(F["tables"][t][0])
    out = dict(st=st, origins=origins, rounds=[])
    totals = [0] * 32
    for r in range(rounds):
        last = r == rounds - 1
        rec = []
        for k, (s, o) in enumerate(zip(sims, origins)):
            a, p = F["tables"][tab[k]]
            q = {}
            s.run_gossip(o)
            q["dist"] = s.distances()
            s.consume_messages(o)
            s.send_prunes(o, THR, MI)
            q["prunes"] = s.prunes()
            totals[k] += len(q["prunes"])
            if last:
                q["caches"] = s.caches(o)
            s.prune_connections()
            q["counters"] = tuple(np.where(x == U64MAX, 0, x) for x in s.counters())
            s.chance_to_rotate(a, p, r)
            if last:
                q["pruned_rot"] = s.pruned_all(o)
            rec.append(q)
        out["rounds"].append(rec)
    out["entries"] = [sims[8 * t].entries(F["tables"][t][0]) for t in range(4)]
    out["totals"] = totals
    return out


def test_case_f_straddling_table():
    t = f_trace()
    assert t["totals"] == F["prunes"] and min(t["totals"]) > 0, t["totals"]  # (the oracle alone)
    assert t["origins"][0] == t["origins"][1] == t["origins"][8] and t["origins"][9] == t["origins"][24]
    assert len(set(t["origins"])) == 29
    eng = gs.Engine(t["st"], 32, fanout=6, seed=SEED, trajectories=[(a, p, 8) for a, p in F["tables"]], **MULTI)
    eng.set_slots(t["origins"], MI, THR)
    eng.init_active_sets()
    geo = eng.bfs_geometry()  # (the groups exist once the slots are set)
    assert _is_multi(eng) and geo["group_width"] == 28 and geo["groups"] == 2
    for r, rec in enumerate(t["rounds"]):
        eng.round(r, record=True)
        for k, q in enumerate(rec):
            msg = f"F slot {k} round {r}"
            np.testing.assert_array_equal(eng.distances(k), q["dist"], err_msg="hops " + msg)
            assert eng.prunes(k) == q["prunes"], "prunes " + msg
            for got, want in zip(eng.counters(k), q["counters"]):
                np.testing.assert_array_equal(got, want, err_msg="counters " + msg)
    for k, q in enumerate(t["rounds"][-1]):
        tt.assert_caches(eng, k, q["caches"], f"caches F slot {k}")
        np.testing.assert_array_equal(eng.pruned_all(k), q["pruned_rot"], err_msg=f"prune state F slot {k}")
    tt.assert_entries(eng, t["entries"])
    assert eng.info()["bfs_persistent"]


# ------------------------------------------------ 3. no sharing inside a group ----
def _round_readbacks(eng, S):
    out = []
    for k in range(S):
        out += [eng.hops(k), np.array(eng.prunes(k), dtype=np.uint32).reshape(-1, 2), *eng.counters(k),
                eng.pruned_all(k), *eng.caches(k)]
    return out


def test_case_g_one_slot_tables_equal_the_workgroup_engine():
    """28 one-slot tables in one group: slots of different tables share no frontier entry and no
    push record, so a pool or queue capacity that still assumed shared records would end in
    GS_ERANGE (raised by the readbacks) or in different results."""
    n, S, rounds = 400, 28, 25
    _, st = eb.synth.network(n)
    sizes = [6 + (k % 27) for k in range(S)]
    tabs = [(a, .05, 1) for a in sizes]
    origins = [(k * 14 + 3) % n for k in range(S)]

    def run(**kw):
        eng = gs.Engine(st, S, fanout=6, seed=SEED, trajectories=tabs, **kw)
        eng.set_slots(origins, MI, THR)
        eng.init_active_sets()
        per_round = []
        for r in range(rounds):
            eng.round(r, record=True)
            per_round.append(_round_readbacks(eng, S))
        eng.sync()
        return eng, per_round, [eng.active_sets(table=t) for t in range(S)], eng.summaries()

    wg, want, want_ent, want_sum = run()
    assert wg.info()["bfs_mode"] == gs.GS_BFS_WORKGROUP
    wg.close()
    eng, got, got_ent, got_sum = run(**MULTI)
    assert _is_multi(eng) and eng.bfs_geometry()["groups"] == 1 and eng.info()["bfs_persistent"]
    for r in range(rounds):
        for i, (x, y) in enumerate(zip(got[r], want[r])):
            np.testing.assert_array_equal(x, y, err_msg=f"G round {r} readback {i}")
    for t in range(S):
        for x, y in zip(got_ent[t], want_ent[t]):
            np.testing.assert_array_equal(x, y, err_msg=f"G entries table {t}")
    np.testing.assert_array_equal(got_sum, want_sum)
    assert int(want_sum["prunes"].sum(axis=0).min()) > 0  # (every slot pruned: no idle prune path)


# ------------------------------------------------ 4. beyond the workgroup engine ----
def _digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def test_tables_equal_single_table_engines_at_20000_nodes():
    """No debug flags: levels outgrow the small-level kernel. Every round's hops, prunes, counters,
    caches, prune state and entries, as digests (equal digests, equal arrays). 24 rounds: prunes
    need 20 upserts."""
    n, per, rounds = 20000, 2, 24
    tabs = [(12, .01), (20, .01), (27, .05)]
    assert not gs.traj_supported(n, 6, 27)[0] and gs.traj_multi_supported(n, 6, 6, 27)
    st = eb.synth.power_law_stakes(n)  # (id order is irrelevant to an engine-to-engine comparison)
    order = np.argsort(-st.astype(np.int64), kind="stable")
    org = [int(order[0]), int(order[49])]  # origin ranks 1 and 50

    def run(eng, origins, tables):
        """-> {(table, slot in table, round): digest}, prunes summed over rounds per slot."""
        eng.set_slots(origins, MI, THR)
        eng.init_active_sets()
        out, total = {}, [0] * len(origins)
        for r in range(rounds):
            eng.round(r, record=True)
            for k in range(len(origins)):
                t = k // per if len(tables) > 1 else 0
                pr = eng.prunes(k)
                total[k] += len(pr)
                out[(tables[t], k % per, r)] = _digest(eng.hops(k), np.array(pr, dtype=np.uint32), *eng.counters(k),
                                                      *eng.caches(k), eng.pruned_all(k))
            for t in range(len(tables)):
                out[(tables[t], "entries", r)] = _digest(*eng.active_sets(table=t))
        return out, total, eng.summaries()

    multi = gs.Engine(st, per * len(tabs), fanout=6, seed=SEED, trajectories=[(a, p, per) for a, p in tabs], **MULTI)
    assert _is_multi(multi) and multi.info()["bfs_persistent"]
    got, got_total, ms = run(multi, org * len(tabs), tabs)
    multi.close()
    assert min(got_total) > 0, got_total
    for t, (a, p) in enumerate(tabs):
        one = gs.Engine(st, per, fanout=6, seed=SEED, active_set_size=a, rotation_probability=p, bfs_mode=gs.GS_BFS_MULTI)
        want, want_total, os_ = run(one, org, [(a, p)])
        one.close()
        assert want_total == got_total[t * per:(t + 1) * per]
        for key, d in want.items():
            assert got[key] == d, f"table {t} {key}"
        np.testing.assert_array_equal(ms[:, t * per:(t + 1) * per], os_, err_msg=f"summaries table {t}")


# ------------------------------------------------ 5. refusals and round trip ----
def test_refusals_auto_and_round_trip():
    _, st = eb.synth.network(100)
    tr = [(12, .25, 1), (8, .5, 2)]

    def make(tr=tr, n_slots=3, st=st, **kw):
        return gs.Engine(st, n_slots, fanout=6, seed=SEED, trajectories=tr, **kw)

    for mode in (gs.GS_BFS_LEVEL, gs.GS_BFS_BINNED, gs.GS_BFS_HYBRID):
        with pytest.raises(gs.GsError) as ei:
            make(bfs_mode=mode, traj_multi=True)
        assert ei.value.code == -1
    with pytest.raises(gs.GsError) as ei:  # without the flag MULTI is still refused, with the old message
        make(bfs_mode=gs.GS_BFS_MULTI)
    assert ei.value.code == -1 and "GS_BFS_WORKGROUP" in str(ei.value)
    # AUTO with the flag: WORKGROUP where the workgroup engine fits, else MULTI (create only)
    small = make([(12, .1, 1), (8, .1, 1)], n_slots=2, traj_multi=True)
    assert small.info()["bfs_mode"] == gs.GS_BFS_WORKGROUP
    small.close()
    big = make([(12, .1, 1), (8, .1, 1)], n_slots=2, st=np.full(70000, 10**9, dtype=np.uint64), traj_multi=True)
    assert big.info()["bfs_mode"] == gs.GS_BFS_MULTI and big.trajectories() == [(12, .1, 1), (8, .1, 1)]
    other = big.info()["other_bytes"]
    big.close()
    one = gs.Engine(np.full(70000, 10**9, dtype=np.uint64), 2, fanout=6, seed=SEED, active_set_size=12,
                    bfs_mode=gs.GS_BFS_MULTI)
    assert other > one.info()["other_bytes"]  # (the table bank is counted under other_bytes)
    one.close()
    # one table with the flag is exactly gs_create in that mode
    solo = make([(12, .25, 3)], bfs_mode=gs.GS_BFS_MULTI, traj_multi=True)
    assert solo.info()["bfs_mode"] == gs.GS_BFS_MULTI and solo.trajectories() == [(12, .25, 3)]
    solo.close()

    # the round trip of an uploaded entry, side by side with a workgroup table engine
    def prepared(**kw):
        eng = make(**kw)
        eng.set_slots([1, 2, 3], MI, THR)
        eng.init_active_sets()
        for r in range(25):
            eng.round(r)
        return eng

    wg = prepared()
    wg_before = [wg.pruned_all(k) for k in range(3)]
    node = int(np.argmax(wg_before[1] | wg_before[2]))
    assert (wg_before[1] | wg_before[2])[node] and wg_before[0].any()
    new = [(node + 1) % 100, (node + 2) % 100]
    for b in range(25):
        wg.set_entry(node, b, new, table=1)
    wg.round(25, record=True)
    want = _round_readbacks(wg, 3) + [wg.active_sets(table=t)[0] for t in range(2)]
    assert wg.info()["bfs_mode"] == gs.GS_BFS_WORKGROUP
    wg.close()
    eng = prepared(**MULTI)
    assert _is_multi(eng) and eng.trajectories() == tr
    for call in (eng.active_sets, lambda: eng.get_entry(3, 0), lambda: eng.set_entry(3, 0, [1, 2])):
        with pytest.raises(gs.GsError) as ei:
            call()
        assert ei.value.code == -1 and "_traj" in str(ei.value)
    before = [eng.pruned_all(k) for k in range(3)]
    for x, y in zip(before, wg_before):
        np.testing.assert_array_equal(x, y)
    for b in range(25):
        eng.set_entry(node, b, new, table=1)
    assert eng.get_entry(node, 3, table=1) == new
    after = [eng.pruned_all(k) for k in range(3)]
    np.testing.assert_array_equal(after[0], before[0])  # table 0's slot keeps its prune bits
    assert after[1][node] == 0 and after[2][node] == 0
    eng.round(25, record=True)
    got = _round_readbacks(eng, 3) + [eng.active_sets(table=t)[0] for t in range(2)]
    for i, (x, y) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(x, y, err_msg=f"readback {i} after the upload")
    eng.sync()


# ------------------------------------------------ 6. above the engine ----
from test_slot_fanout import F64_NAMES, U64_NAMES  # noqa: E402


def test_run_simulations_on_the_multi_table_engine():
    """Non-adjacent equal (size, probability) pairs; every result name equals the per-value runs.
    20 warm-up rounds and 10 recorded ones: `iterations` counts the warm-up rounds too, so it is
    30 (10 would record nothing and every name would compare empty), and the recorded rounds
    20..29 are the ones in which cache entries reach their 20th upsert and prune."""
    _, st = eb.synth.network(150)
    aszs, probs, ranks = [8, 12, 8, 12], [.02, .3, .02, .3], [1, 1, 2, 2]
    res = gs.run_simulations(st, n_sims=4, aszs=aszs, rot_probs=probs, origin_ranks=ranks, iterations=30, warm_up=20,
                             seed=9, bfs_mode=gs.GS_BFS_MULTI)
    for k, (a, p, rk) in enumerate(zip(aszs, probs, ranks)):
        one = gs.run_simulations(st, n_sims=1, asz=a, p=p, origin_ranks=[rk], iterations=30, warm_up=20, seed=9,
                                 bfs_mode=gs.GS_BFS_MULTI)
        assert len(one.f64(0, "coverage")) == 10 and one.u64(0, "prune_hist").sum() > 0
        for name in F64_NAMES:
            np.testing.assert_array_equal(res.f64(k, name), one.f64(0, name), err_msg=f"sim {k} {name}")
        for name in U64_NAMES:
            np.testing.assert_array_equal(res.u64(k, name), one.u64(0, name), err_msg=f"sim {k} {name}")


def test_run_traj_sweep_multi_equals_run_sweep():
    """17,000 nodes do not fit the workgroup engine: with multi=True the share is one engine."""
    import gossip_sim_amd.sweep as sw
    st = eb.synth.power_law_stakes(17000)
    sizes, calls = [9, 14], []

    def runner(stakes, **kw):
        calls.append((kw["n_sims"], kw.get("bfs_mode")))
        return gs.run_simulations(stakes, **kw)

    def cfg(a):
        return dict(asz=a, iterations=8, warm_up=3, seed=4)

    a = sw.run_traj_sweep(st, sizes, cfg, runner=runner, multi=True)
    assert calls == [(2, gs.GS_BFS_MULTI)]  # one engine
    b = sw.run_sweep(st, sizes, cfg)
    for i in range(2):
        for kind, name in sw.NAMES:
            np.testing.assert_array_equal(a.per_sim[i][(kind, name)], b.per_sim[i][(kind, name)], err_msg=name)
    del calls[:]
    sw.run_traj_sweep(st, sizes, cfg, runner=runner)  # multi=False: nothing changes
    assert calls == [(1, None), (1, None)]


# -------------------------------------------------------------------- CLI ----
from test_cli import F64_NAMES as CLI_F64, U64_NAMES as CLI_U64, cli, oracle_sims, sweep_params, yaml_net  # noqa: E402,F401
import report_ref as rr  # noqa: E402


@pytest.mark.parametrize("kind", ["active-set-size", "rotate-probability"])
def test_cli_batch_sweeps_bfs_mode_4(kind, yaml_net, tmp_path):
    """--batch-sweeps --bfs-mode 4 on the 60-node network: one multi-source table engine; results
    equal to the oracle's per sim, the report unchanged, the plan one line of lists."""
    path, keys, st, pks = yaml_net
    iters, warm, seed = 34, 6, 13
    test_type, step = (1, 2) if kind == "active-set-size" else (7, 0.25)
    params = sweep_params(test_type, 3, iterations=iters, warm_up=warm, step=step)
    res, plan = str(tmp_path / "g.txt"), str(tmp_path / "plan.txt")
    r = cli("--accounts-from-yaml", "--account-file", path, "--iterations", iters, "--warm-up-rounds", warm,
            "--test-type", kind, "--step-size", step, "--num-simulations", 3, "--origin-rank", 1, 1, 1, 1,
            "--print-stats", "--save-results", res, "--seed", seed, "--engine-plan", plan, "--batch-sweeps",
            "--bfs-mode", 4)
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
