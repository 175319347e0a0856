"""Round split (GS_ROUND_SPLIT): gs_round launches the slots as two groups on two
streams, one round apart at most, over three generations of rows and rotation lists.

Every case runs the same engine twice, split forced on (GS_ROUND_SPLIT=force: the slot floor
that keeps small engines on one stream is dropped) and off (GS_ROUND_SPLIT=0), and compares
everything the round leaves behind byte for byte: the recorded summaries, hops, counters,
accumulators, caches (meta, keys, scores), prune masks and the rows read back after the run.
The rotation probability is high, so the rows change every round and a launch that read or
wrote the wrong generation would show.
"""
import contextlib
import os

import numpy as np
import pytest

import engine_bind as eb
import oracle_bind as ob

gs = eb.gs
pytestmark = pytest.mark.gpu
THR, MI = 0.15, 2


@contextlib.contextmanager
def round_split(value):
    old = os.environ.get("GS_ROUND_SPLIT")
    os.environ["GS_ROUND_SPLIT"] = value
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("GS_ROUND_SPLIT", None)
        else:
            os.environ["GS_ROUND_SPLIT"] = old


def spread_origins(st, S):
    order = np.argsort(np.asarray(st, dtype=np.uint64), kind="stable")
    return [int(order[(k * (len(order) - 1)) // max(1, S - 1)]) for k in range(S)]


def engine_pair(st, S, *, p, seed, want_split=True, **kw):
    """(split, single): the same engine with the split forced and with it off."""
    out = []
    for value in ("force", "0"):
        with round_split(value):  # (read at creation)
            out.append(gs.Engine(st, S, seed=seed, rotation_probability=p, bfs_mode=gs.GS_BFS_WORKGROUP, **kw))
    a, b = out
    assert a.info()["fused_round"] and b.info()["fused_round"]
    assert not b.info()["round_split"] and b.info()["round_split_groups"] == []
    if want_split:
        g = a.info()["round_split_groups"]
        assert a.info()["round_split"] and len(g) == 2 and min(g) >= 1 and sum(g) == S, g
        assert abs(g[0] - g[1]) <= 1
    else:
        assert not a.info()["round_split"]
    return a, b


def assert_same(a, b, S, tag):
    np.testing.assert_array_equal(a.summaries(), b.summaries(), err_msg=f"summaries {tag}")
    for k in range(S):
        np.testing.assert_array_equal(a.hops(k), b.hops(k), err_msg=f"hops slot {k} {tag}")
        for nm, x, y in zip(("egress", "cnt", "prunes"), a.counters(k), b.counters(k)):
            np.testing.assert_array_equal(x, y, err_msg=f"counters {nm} slot {k} {tag}")
        for x, y in zip(a.accumulators(k), b.accumulators(k)):
            np.testing.assert_array_equal(x, y, err_msg=f"accumulators slot {k} {tag}")
        for nm, x, y in zip(("upserts", "len", "keys", "scores"), a.caches(k), b.caches(k)):
            np.testing.assert_array_equal(x, y, err_msg=f"cache {nm} slot {k} {tag}")
        np.testing.assert_array_equal(a.pruned_all(k), b.pruned_all(k), err_msg=f"prune masks slot {k} {tag}")
    for nm, x, y in zip(("peers", "lens"), a.active_sets(), b.active_sets()):
        np.testing.assert_array_equal(x, y, err_msg=f"rows {nm} {tag}")


@pytest.mark.parametrize("S", [2, 9])
def test_rows_change_every_round(S):
    """N = 300, rotation probability 0.2, 26 rounds (past the first prune wave), nothing read
    back before the end: the groups run as far apart as the events allow. S = 9 splits 5 + 4."""
    n, seed, p = 300, 31, 0.2
    _, st = eb.synth.network(n)
    a, b = engine_pair(st, S, p=p, seed=seed)
    origins = spread_origins(st, S)
    for e in (a, b):
        e.set_slots(origins, MI, THR)
        e.init_active_sets()
        for r in range(26):
            e.round(r, record=True)
    assert_same(a, b, S, f"S {S}")
    assert a.summaries().shape[0] == 26 and int(a.summaries()["prunes"].sum()) > 0
    for e in (a, b):
        e.close()


def test_record_toggled_per_round():
    """N = 64, S = 5, every other round recorded: each group writes its own slots of the row
    the ring index names, and the index moves once per recorded round."""
    n, S, seed, p = 64, 5, 7, 0.2
    _, st = eb.synth.network(n)
    a, b = engine_pair(st, S, p=p, seed=seed)
    origins = spread_origins(st, S)
    for e in (a, b):
        e.set_slots(origins, MI, THR)
        e.init_active_sets()
        for r in range(26):
            e.round(r, record=r % 2 == 0)
    assert a.summaries().shape[0] == 13
    assert_same(a, b, S, "toggled record")
    for e in (a, b):
        e.close()


def test_joins_and_row_changes_mid_run():
    """N = 300, S = 9: failed nodes before round 0, a hops readback after every third round (the
    primary stream joins the other mid-run) and an uploaded entry at round 7 (the rows change
    in place: the generations are made equal again before the next round)."""
    n, S, seed, p = 300, 9, 13, 0.2
    _, st = eb.synth.network(n)
    a, b = engine_pair(st, S, p=p, seed=seed)
    origins = spread_origins(st, S)
    node = origins[S // 2]
    for e in (a, b):
        e.set_slots(origins, MI, THR)
        e.init_active_sets()
        e.fail_nodes([0.1] * S)
    for r in range(26):
        for e in (a, b):
            if r == 7:
                row = e.get_entry(node, 0)
                assert len(row) >= 2
                e.set_entry(node, 0, row[::-1])
            e.round(r, record=True)
        if r % 3 == 2:
            for k in (0, S - 1):
                np.testing.assert_array_equal(a.hops(k), b.hops(k), err_msg=f"hops slot {k} round {r}")
    assert_same(a, b, S, "joins")
    assert int(a.summaries()["prunes"].sum()) > 0
    for e in (a, b):
        e.close()


def test_per_slot_fanouts():
    """N = 300, S = 6 with fanouts that differ (the per-slot-fanout kernel): the group's fanout
    array starts at its first slot like every other per-slot array."""
    n, S, seed, p = 300, 6, 19, 0.2
    _, st = eb.synth.network(n)
    a, b = engine_pair(st, S, p=p, seed=seed)
    origins = spread_origins(st, S)
    for e in (a, b):
        e.set_slots(origins, MI, THR)
        e.set_slot_fanouts([6 - k % 3 for k in range(S)])
        e.init_active_sets()
        for r in range(26):
            e.round(r, record=True)
    assert_same(a, b, S, "per-slot fanouts")
    for e in (a, b):
        e.close()


def test_split_round_matches_oracle():
    """2 slots (one per group), 24 rounds at rotation probability 0.05 against the oracle round by
    round: hops and prunes of both slots. The oracle alone, on the CPU, first prunes at round 19
    for both origins with this seed (2,948 prunes in the 24 rounds); the test counts them."""
    n, seed, p, asz = 300, 23, 0.05, 12
    pks, st = eb.synth.network(n)
    origins = spread_origins(st, 2)
    with round_split("force"):
        eng = gs.Engine(st, 2, seed=seed, active_set_size=asz, rotation_probability=p, bfs_mode=gs.GS_BFS_WORKGROUP)
    assert eng.info()["round_split"] and eng.info()["round_split_groups"] == [1, 1]
    eng.set_slots(origins, MI, THR)
    eng.init_active_sets()
    sims = [ob.Sim(ob.PHILOX, seed, pks, st, 6) for _ in origins]
    for s in sims:
        s.init_philox(asz)
    prunes = 0
    for r in range(24):
        eng.round(r)
        for k, (s, o) in enumerate(zip(sims, origins)):
            s.run_gossip(o)
            s.consume_messages(o)
            s.send_prunes(o, THR, MI)
            np.testing.assert_array_equal(eng.distances(k), s.distances(), err_msg=f"hops slot {k} round {r}")
            assert eng.prunes(k) == s.prunes(), f"prunes slot {k} round {r}"
            prunes += len(s.prunes())
            s.prune_connections()
            s.chance_to_rotate(asz, p, r)
    assert prunes > 0, "the oracle pruned nothing: the case tests nothing"
    for k, (s, o) in enumerate(zip(sims, origins)):
        np.testing.assert_array_equal(eng.pruned_all(k), s.pruned_all(o), err_msg=f"prune state slot {k}")
    eng.close()


def test_ineligible_engines_stay_on_one_stream():
    """Several trajectory tables, the cluster view and a single slot: the split reports off even
    when forced, and the rounds equal those of the engine created with it off."""
    n, seed, p = 64, 5, 0.2
    _, st = eb.synth.network(n)
    cases = [dict(S=4, kw=dict(trajectories=[(12, p, 2), (8, 0.1, 2)]), cluster=False),
             dict(S=4, kw=dict(), cluster=True),
             dict(S=1, kw=dict(), cluster=False)]
    for c in cases:
        S = c["S"]
        a, b = engine_pair(st, S, p=p, seed=seed, want_split=c["cluster"], **c["kw"])
        origins = spread_origins(st, S)
        for e in (a, b):
            e.set_slots(origins, MI, THR)
            e.init_active_sets()
            if c["cluster"]:
                e.enable_cluster_view(True)
            assert not e.info()["round_split"]
            for r in range(8):
                e.round(r, record=True)
        np.testing.assert_array_equal(a.summaries(), b.summaries())
        for k in range(S):
            np.testing.assert_array_equal(a.hops(k), b.hops(k))
            np.testing.assert_array_equal(a.pruned_all(k), b.pruned_all(k))
        for e in (a, b):
            e.close()
