#!/usr/bin/env python3
"""What the delivery tree's view in stake costs per recorded round:
kernel_time("tree_stake") beside kernel_time("tree") and kernel_time("round") of the same engine,
on the C2 shape (3,000 nodes, all origins, the one-kernel round), with one group and with one
group per slot, twice each. Every round is recorded; one JSON line per run. The last round's view
is checked first on 16 sampled slots: the per-slot below against a Python walk of Engine.tree, and
with per-slot groups the group's last_below against it.
--records: the view's records mode at 100,000 nodes and 16 slots on the
multi-source BFS with the records tree: "tree_stake" and "tree" time and launches per recorded
round, and the launches a walk of one launch per level would have had; two slots are checked.
--dominators: the dominator kind at the same shape, beside the records mode."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import engine_bind as eb

gs, synth = eb.gs, eb.synth


def run(per_slot, warmup=20, steps=100):
    n = s = 3000
    _, st = synth.network(n)
    eng = gs.Engine(st, s, seed=0x5EED0003, active_set_size=12, rotation_probability=0.013333,
                    bfs_mode=gs.GS_BFS_WORKGROUP, profile=True)
    eng.set_slots(list(range(n)))
    eng.enable_tree()
    eng.enable_tree_stake(groups=[1] * s if per_slot else None)
    eng.init_active_sets()
    for r in range(warmup):
        eng.round(r, record=True)
    eng.sync()
    eng.kernel_time_reset()
    for r in range(warmup, warmup + steps):
        eng.round(r, record=True)
    eng.sync()
    fam = {f: eng.kernel_time(f) for f in ("tree_stake", "tree", "round")}
    sti = [int(x) for x in st]
    for j in range(0, s, s // 16):
        parent, hops = eng.tree(j).tolist(), eng.hops(j).tolist()
        below = [0] * n
        for w in sorted((w for w in range(n) if parent[w] != 0xFFFFFFFF), key=lambda w: -hops[w]):
            below[parent[w]] += below[w] + sti[w]
        assert [int(x) for x in eng.tree_stake(j)] == below, j
        if per_slot:
            assert list(eng.tree_stake_load(j)["last_below"]) == below, j
    assert eng.tree_stake_load()["rounds"] == warmup + steps
    out = {"per_slot_groups": per_slot, "steps": steps,
           "tree_stake_us_per_round": round(1e3 * fam["tree_stake"][0] / steps, 2),
           "tree_stake_launches": fam["tree_stake"][1],
           "tree_us_per_round": round(1e3 * fam["tree"][0] / steps, 2),
           "round_us_per_round": round(1e3 * fam["round"][0] / steps, 2)}
    print(json.dumps(out), flush=True)
    eng.close()


def below_of(eng, j, sti):
    parent, hops = eng.tree(j).tolist(), eng.hops(j).tolist()
    below = [0] * len(sti)
    for w in sorted((w for w in range(len(sti)) if parent[w] != 0xFFFFFFFF), key=lambda w: -hops[w]):
        below[parent[w]] += below[w] + sti[w]
    return below, max(h for h in hops if h < 255)


def run_records(n=100_000, s=16, warmup=10, steps=100):
    _, st = synth.network(n)
    eng = gs.Engine(st, s, seed=0x5EED0003, active_set_size=12, rotation_probability=0.013333,
                    bfs_mode=gs.GS_BFS_MULTI, profile=True)
    eng.set_slots([j * (n // s) for j in range(s)])
    eng.enable_tree(records=True)
    eng.enable_tree_stake(groups=[1] * s, records=True)
    eng.init_active_sets()
    for r in range(warmup):
        eng.round(r, record=True)
    eng.sync()
    eng.kernel_time_reset()
    for r in range(warmup, warmup + steps):
        eng.round(r, record=True)
    eng.sync()
    fam = {f: eng.kernel_time(f) for f in ("tree_stake", "tree", "tree.kernels", "bfs")}
    sti, depth = [int(x) for x in st], 0
    for j in range(s):
        if j in (0, s - 1):
            below, d = below_of(eng, j, sti)
            assert [int(x) for x in eng.tree_stake(j)] == below, j
            assert list(eng.tree_stake_load(j)["last_below"]) == below, j
        else:
            d = int(eng.hops(j)[eng.hops(j) < 255].max())
        depth = max(depth, d)
    print(json.dumps({"records": True, "nodes": n, "slots": s, "steps": steps,
                      "tree_stake_us_per_round": round(1e3 * fam["tree_stake"][0] / steps, 2),
                      "tree_stake_launches_per_round": fam["tree_stake"][1] / steps,
                      "last_round_levels": depth, "last_round_launches_one_per_level": depth + 3,
                      "tree_us_per_round": round(1e3 * fam["tree"][0] / steps, 2),
                      "tree_kernels_last_round": fam["tree.kernels"][1],
                      "bfs_us_per_round": round(1e3 * fam["bfs"][0] / steps, 2)}), flush=True)
    eng.close()


def run_dominators(n=100_000, s=16, warmup=10, steps=50):
    """The dominator kind at the records mode's shape, beside the first-delivery
    walk of an identical engine: both kinds' "tree_stake" and "tree" per recorded round, and the
    sweeps per round (read after every round: a host wait outside the timed launches). Checked on
    slot 0: below of the origin is every reached stake, and no node is below more stake in the
    dominator tree than in the first-delivery tree."""
    _, st = synth.network(n)
    out = {"dominators": True, "nodes": n, "slots": s, "steps": steps}
    below = {}
    for kind in ("records", "dominators"):
        eng = gs.Engine(st, s, seed=0x5EED0003, active_set_size=12, rotation_probability=0.013333,
                        bfs_mode=gs.GS_BFS_MULTI, profile=True)
        eng.set_slots([j * (n // s) for j in range(s)])
        eng.enable_tree(records=True)
        eng.enable_tree_stake(groups=[1] * s, records=True, dominators=kind == "dominators")
        eng.init_active_sets()
        sweeps = []
        for r in range(warmup + steps):
            if r == warmup:
                eng.sync()
                eng.kernel_time_reset()
            eng.round(r, record=True)
            if kind == "dominators" and r >= warmup:
                sweeps.append(eng.kernel_time("tree_stake.sweeps")[1])
        eng.sync()
        fam = {f: eng.kernel_time(f) for f in ("tree_stake", "tree")}
        below[kind] = eng.tree_stake(0)
        out[kind + "_tree_stake_us_per_round"] = round(1e3 * fam["tree_stake"][0] / steps, 2)
        out[kind + "_tree_stake_launches_per_round"] = fam["tree_stake"][1] / steps
        out[kind + "_tree_us_per_round"] = round(1e3 * fam["tree"][0] / steps, 2)
        if sweeps:
            out["sweeps_per_round_mean"], out["sweeps_per_round_max"] = sum(sweeps) / len(sweeps), max(sweeps)
            idom, parent = eng.dominators(0), eng.tree(0)
            out["slot0_idom_not_parent"] = int((idom != parent).sum())
            out["slot0_idom_not_parent_nor_origin"] = int(((idom != parent) & (idom != 0)).sum())
        eng.close()
    assert below["records"][0] == below["dominators"][0] > 0  # (slot 0's origin is node 0)
    assert (below["dominators"] <= below["records"]).all()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    if "--dominators" in sys.argv[1:]:
        run_dominators()
        sys.exit(0)
    if "--records" in sys.argv[1:]:
        run_records()
        sys.exit(0)
    for rep in range(2):
        run(False)
        run(True)
