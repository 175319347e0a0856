"""The fixtures of tests/test_degenerate_graphs.py: a chain of a chosen depth, the engine
variants that reach each BFS implementation's hop-limit guard, and the oracle's rounds on
the chain (computed once per case and shared).

chain_case(D): n = D + 1 + spare nodes of equal stake (one stake bucket, so every node
uses the same entry k = min(bucket[u], bucket[origin]) for every origin), pubkeys of
synth.network(n). A seeded permutation c of the ids carries the chain, so it does not run
in id order (the multi / binned BFS's destination bins, the consume tie-break). Node c[i],
0 <= i <= D, holds the peers [c[i+1] (while i < D), c[i-1], c[i-2]] (out-of-range ones
dropped) in all 25 entries; the spare nodes hold nothing and are never pushed to. Push
fanout 3, active-set size 12, rotation probability 0: the graph is the same every round
except for what pruning removes. From the origin c[0], c[i] is at distance i, every level
holds one node, and c[i] receives from c[i-1] (hop i), c[i+1] (hop i + 2) and c[i+2]
(hop i + 3): at D = 253 the record c[253] -> c[252] carries hop 254, the largest a u8
record may hold."""
import functools

import numpy as np

import engine_bind as eb
import oracle_bind as ob

gs = eb.gs
FANOUT, ASZ, SEED = 3, 12, 19
STAKE = 1_000_000 * 10**9  # lamports; the same for every node
U64MAX = np.uint64(2**64 - 1)


@functools.lru_cache(maxsize=None)
def chain_case(D, spare=40, seed=5):
    n = D + 1 + spare
    pks, _ = eb.synth.network(n)
    c = [int(x) for x in np.random.default_rng(seed).permutation(n)]
    peers = np.zeros((n, 25, ASZ), dtype=np.uint32)
    lens = np.zeros((n, 25), dtype=np.uint8)
    lists = {}
    for i in range(D + 1):
        lst = ([c[i + 1]] if i < D else []) + [c[j] for j in (i - 1, i - 2) if j >= 0]
        lists[c[i]] = lst
        peers[c[i], :, :len(lst)] = lst
        lens[c[i], :] = len(lst)
    return dict(D=D, n=n, spare=spare, pks=pks, stakes=np.full(n, STAKE, dtype=np.uint64), c=c, lists=lists,
                peers=peers, lens=lens)


def chain_sim(case):
    """The oracle on the chain (one Sim serves one origin)."""
    s = ob.Sim(ob.PHILOX, SEED, case["pks"], case["stakes"], FANOUT)
    s.set_entries(case["peers"], case["lens"])
    return s


def chain_engine(case, n_slots, **kw):
    """The engine on the chain: every (node, bucket) entry uploaded, no init_active_sets."""
    eng = gs.Engine(case["stakes"], n_slots, fanout=FANOUT, active_set_size=ASZ, rotation_probability=0.0, seed=SEED,
                    **kw)
    for node, lst in case["lists"].items():
        for k in range(25):
            eng.set_entry(node, k, lst)
    return eng


@functools.lru_cache(maxsize=None)
def chain_rounds(D, rounds, mi=2, thr=0.15, every=False):
    """The oracle's `rounds` rounds on chain_case(D) from the origins c[0] and c[1]: per
    round and slot the distances, the orders CSR, the prune set and the counters; caches
    and prune state after the last round (after every round with `every`). Read-only."""
    case = chain_case(D)
    origins = case["c"][:2]
    sims = [chain_sim(case) for _ in origins]
    out = []
    for r in range(rounds):
        rec = []
        for s, o in zip(sims, origins):
            q = {}
            s.run_gossip(o)
            q["dist"] = s.distances()
            q["orders"] = s.orders_all(64 * case["n"])
            s.consume_messages(o)
            s.send_prunes(o, thr, mi)
            q["prunes"] = s.prunes()
            if every or r == rounds - 1:
                q["caches"] = s.caches(o)
            s.prune_connections()
            q["counters"] = s.counters()
            if every or r == rounds - 1:
                q["pruned"] = s.pruned_all(o)
            s.chance_to_rotate(ASZ, 0.0, r)
            for a in q.values():
                for x in (a if isinstance(a, tuple) else (a,)):
                    if isinstance(x, np.ndarray):
                        x.setflags(write=False)
            rec.append(q)
        out.append(rec)
    return out


def summary_of(q, n):
    """gs_round_summary's integer fields of one slot's round, from the oracle's distances
    (and its record count): no node fails on the chain, so every unreached node is stranded."""
    d = q["dist"]
    reached = d != U64MAX
    h = np.sort(d[reached & (d != 0)].astype(np.int64))
    c = len(h)
    return dict(visited=int(reached.sum()), pushes=len(q["orders"][1]), prunes=len(q["prunes"]),
                stranded=int(n - reached.sum()), hop_sum=int(h.sum()), hop_count=c, hop_min=int(h[0]),
                hop_max=int(h[-1]), hop_med_lo=int(h[(c - 1) // 2]), hop_med_hi=int(h[c // 2]))


# The engine variants, one per hop-limit guard. `env`: set before the engine is created
# (pb_setup in gs_bfs_pers.hip reads GS_MV_PBFS at every engine creation, not once per
# process, so the variants need no order and no process of their own). `fused`: the engine's
# gs_round is the one-kernel round. `steps`: the step-wise calls instead of gs_round.
VARIANTS = {
    "wg-fused": dict(kw=dict(bfs_mode=gs.GS_BFS_WORKGROUP), fused=True),
    "wg-split": dict(kw=dict(bfs_mode=gs.GS_BFS_WORKGROUP, split_round=True)),
    "wg-steps": dict(kw=dict(bfs_mode=gs.GS_BFS_WORKGROUP), fused=True, steps=True),
    "level": dict(kw=dict(bfs_mode=gs.GS_BFS_LEVEL)),
    "binned-small": dict(kw=dict(bfs_mode=gs.GS_BFS_BINNED, binned_all_levels=False)),
    "binned-all": dict(kw=dict(bfs_mode=gs.GS_BFS_BINNED, binned_all_levels=True)),
    "binned-direct": dict(kw=dict(bfs_mode=gs.GS_BFS_BINNED, binned_all_levels=False, no_small_levels=True)),
    "multi": dict(kw=dict(bfs_mode=gs.GS_BFS_MULTI)),
    "multi-loop": dict(kw=dict(bfs_mode=gs.GS_BFS_MULTI), env={"GS_MV_PBFS": "0"}),
    "multi-grid": dict(kw=dict(bfs_mode=gs.GS_BFS_MULTI, no_small_levels=True), env={"GS_MV_PBFS": "0"}),
    "hybrid": dict(kw=dict(bfs_mode=gs.GS_BFS_HYBRID)),
    "hybrid-grid": dict(kw=dict(bfs_mode=gs.GS_BFS_HYBRID, no_small_levels=True)),
}


def variant_engine(name, case, monkeypatch, n_slots=2):
    v = VARIANTS[name]
    for k, x in v.get("env", {}).items():
        monkeypatch.setenv(k, x)
    eng = chain_engine(case, n_slots, **v["kw"])
    for k in v.get("env", {}):
        monkeypatch.delenv(k)
    info = eng.info()
    assert info["bfs_mode"] == v["kw"]["bfs_mode"]
    assert info["fused_round"] == bool(v.get("fused"))
    if "env" in v:
        assert not info["bfs_persistent"]
    return eng


def has_inbound(name):
    """The round leaves its inbound rows readable (the one-kernel round keeps them on-chip)."""
    v = VARIANTS[name]
    return bool(v.get("steps")) or not v.get("fused")


def variant_round(name, eng, r):
    """One recorded round: gs_round, or the step-wise calls and gs_record_round."""
    if VARIANTS[name].get("steps"):
        eng.run_gossip()
        eng.consume_messages()
        eng.send_prunes()
        eng.prune_connections()
        eng.chance_to_rotate(r)
        eng.record_round()
    else:
        eng.round(r, record=True)
