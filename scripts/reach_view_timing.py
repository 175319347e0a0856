#!/usr/bin/env python3
"""What the stake reach view costs per recorded round: kernel_time("reach")
beside kernel_time("cluster") of the unchanged cluster load view in the same engine, on the C2
shape (3,000 nodes, all origins, the one-kernel round), with one group and with one group per
slot, twice each. Both views are on, every round is recorded; one JSON line per run. The last
round's view is checked first: per-slot groups against 32 sampled slots' hops, the one group
against the totals every slot must add up to."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import engine_bind as eb

gs, synth = eb.gs, eb.synth


def run(per_slot, warmup=20, steps=100):
    n = s = 3000
    _, st = synth.network(n)
    eng = gs.Engine(st, s, seed=0x5EED0003, active_set_size=12, rotation_probability=0.013333,
                    bfs_mode=gs.GS_BFS_WORKGROUP, profile=True)
    eng.set_slots(list(range(n)))
    if per_slot:
        eng.enable_reach(groups=[1] * s)
        eng.enable_cluster_view(groups=[1] * s)
    else:
        eng.enable_reach()
        eng.enable_cluster_view()
    eng.init_active_sets()
    for r in range(warmup):
        eng.round(r, record=True)
    eng.sync()
    eng.kernel_time_reset()
    for r in range(warmup, warmup + steps):
        eng.round(r, record=True)
    eng.sync()
    fam = {f: eng.kernel_time(f) for f in ("reach", "cluster", "round")}
    sti = [int(x) for x in st]
    if per_slot:
        for j in range(0, s, s // 32):
            h = eng.hops(j).tolist()
            r = eng.reach(j)
            want_n, want_s = [0] * 256, [0] * 256
            for v, b in enumerate(h):
                want_n[b] += 1
                want_s[b] += sti[v]
            assert [int(x) for x in r["last_nodes"]] == want_n and list(r["last_stake"]) == want_s, j
    else:
        r = eng.reach()
        assert int(r["last_nodes"].sum()) == n * s and sum(r["last_stake"]) == s * sum(sti)
        assert r["rounds"] == warmup + steps
        hist = [int(x) for x in r["last_nodes"]]
        print("last round's node bins:", {b: x for b, x in enumerate(hist) if x}, flush=True)
    out = {"per_slot_groups": per_slot, "steps": steps,
           "reach_us_per_round": round(1e3 * fam["reach"][0] / steps, 2), "reach_launches": fam["reach"][1],
           "cluster_us_per_round": round(1e3 * fam["cluster"][0] / steps, 2),
           "round_us_per_round": round(1e3 * fam["round"][0] / steps, 2)}
    print(json.dumps(out), flush=True)
    eng.close()


if __name__ == "__main__":
    for rep in range(2):
        run(False)
        run(True)
