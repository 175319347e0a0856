#!/usr/bin/env python3
"""What the cluster load view costs per recorded round: an engine with
GS_FLAG_PROFILE and the view on, `--warmup` unrecorded rounds, then `--steps` recorded ones;
kernel_time("cluster") against the round's own families of the same run, and the achieved
bytes/s against the view's byte model (7 B per (slot, node) pair -- hops, egress and prune
bytes, the u32 in-degree -- plus 68 B per node of scratch, totals and peaks, the latter times
the number of groups).

--groups G runs the grouped view (gs_cluster_enable_groups) with G groups of near-equal size,
--weighted with weights 1..7 instead of unit weights; without --groups it is gs_cluster_enable's
view. GS_LIB_VARIANT=name measures gossip-sim_amd/variants/name/libgossip_hip.so instead (an
A/B build, e.g. of the parent commit, for the ungrouped view).

Shapes: c2 = 3,000 synthetic nodes, all 3,000 origins, the one-kernel workgroup round;
        c4 = 1,000,000 power-law nodes, 13 origins, the multi-source BFS (node-major egress).

Prints one JSON line per shape. The last round's view is compared with the sum of the per-slot
readbacks when the shape is small enough to read back (c4; c2 compares 64 sampled slots' sum
bound only), so a timing never comes from a view that is wrong."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def run(shape, warmup, steps, groups=0, weighted=False):
    import numpy as np
    import engine_bind as eb
    gs, synth = eb.gs, eb.synth
    if shape == "c2":
        n, s, mode = 3000, 3000, gs.GS_BFS_WORKGROUP
        _, st = synth.network(n)
        origins = list(range(n))
    else:
        n, s, mode = 1_000_000, 13, gs.GS_BFS_MULTI
        st = synth.power_law_stakes(n)
        origins = [int(x) for x in np.argsort(st)[::-1][:s]]
    eng = gs.Engine(st, s, seed=0x5EED0003, active_set_size=12, rotation_probability=0.013333, bfs_mode=mode,
                    profile=True)
    eng.set_slots(origins)
    G = max(1, groups)
    gsz = [s * (g + 1) // G - s * g // G for g in range(G)]
    w = [j % 7 + 1 if weighted else 1 for j in range(s)]
    if groups:
        eng.enable_cluster_view(groups=gsz, weights=w)
    else:
        eng.enable_cluster_view()
    eng.init_active_sets()
    for r in range(warmup):
        eng.round(r, record=False)
    eng.sync()
    eng.kernel_time_reset()
    t0 = time.perf_counter()
    for r in range(warmup, warmup + steps):
        eng.round(r, record=True)
    eng.sync()
    wall = time.perf_counter() - t0
    fam = {f: eng.kernel_time(f) for f in ("cluster", "round", "bfs", "gather", "gather_consume", "consume", "rotate", "stats")}
    cl_ms, cl_n = fam["cluster"]
    other = sum(ms for f, (ms, _) in fam.items() if f != "cluster")
    model = 7 * n * s + 68 * G * n
    per_round_us = 1e3 * cl_ms / max(1, cl_n)
    # every round's structs against the per-slot summaries (exact), group by group
    sm = eng.summaries()
    lo = 0
    egress = np.zeros(n, dtype=np.uint64)
    for g in range(G):
        cr = eng.cluster_rounds(g if groups else None)
        assert len(cr) == steps == len(sm)
        wg = np.array(w[lo:lo + gsz[g]], dtype=np.uint64)
        for f in ("pushes", "prunes"):
            want = (sm[f][:, lo:lo + gsz[g]].astype(np.uint64) * wg).sum(axis=1)
            assert np.array_equal(cr[f], want), f"group {g}: {f} != weighted sum of slots'"
        egress += eng.cluster_load(g if groups else None)["egress"]
        lo += gsz[g]
    acc = np.zeros(n, dtype=np.uint64)
    for j in (range(s) if s <= 64 else range(0, s, s // 64)):
        acc += np.uint64(w[j]) * eng.accumulators(j)[0]
    ok = np.array_equal(acc, egress) if s <= 64 else bool((acc <= egress).all())
    assert ok, "egress totals disagree with the accumulators"
    out = {"shape": shape, "lib": os.environ.get("GS_LIB_VARIANT", "tree"), "groups": groups, "weighted": weighted,
           "model_fraction_of_8TBps": round(model / (per_round_us * 1e-6) / 8e12, 4), "nodes": n, "slots": s, "recorded_rounds": steps, "cluster_launch_pairs": cl_n,
           "cluster_us_per_round": round(per_round_us, 2), "other_families_us_per_round": round(1e3 * other / steps, 2),
           "families_ms": {f: round(ms, 3) for f, (ms, _) in fam.items()},
           "share_of_round": round(cl_ms / other, 4) if other else None,
           "model_bytes": model, "achieved_GBps": round(model / (per_round_us * 1e-6) / 1e9, 1),
           "wall_ms_per_round": round(1e3 * wall / steps, 3)}
    print(json.dumps(out), flush=True)
    eng.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=["c2", "c4"], required=True)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--groups", type=int, default=0, help="G groups of near-equal size (0: the ungrouped view)")
    ap.add_argument("--weighted", action="store_true", help="weights 1..7 (with --groups)")
    a = ap.parse_args()
    run(a.shape, a.warmup, a.steps, a.groups, a.weighted)
