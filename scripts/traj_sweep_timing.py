#!/usr/bin/env python3
"""An active-set-size / rotation-probability sweep at C2's network (3,000 synthetic nodes,
fanout 6, bench.py's seed and window: 20 warm-up + 100 timed rounds), timed two ways:

  batched    one engine of one trajectory table per value (gs_create_traj)
  pervalue   one single-table engine per value, run back to back (sweep.run_sweep's plan)
  single     one single-table engine of the batched arm's slot count at the largest size
             (the multi-table kernel's per-round cost against the single-table kernel's)

Cases: a = sizes 12..27, one origin each; b = the same sizes, 24 origins each (384 slots);
c = probabilities 0.005 k (k = 1..8) at size 12, one origin each.

One arm per process (`--arm`): prints a JSON line with the device-synchronised wall time of
the timed rounds (summed over the engines of the per-value arm) and a digest per slot of
hops, prune state, caches and recorded summaries. `--drive` runs the arms as child processes,
alternating, `--reps` times each, checks that the arms' digests agree slot for slot and prints
one summary line per case. `--pervalue-tree DIR` runs the per-value arm from another built
checkout of this repository (its package and library), e.g. the parent commit's.
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, NODES, FANOUT = 0x5EED0003, 3000, 6


def case_values(case):
    """(size, probability, origins) per value."""
    if case == "a":
        return [(a, 0.01, [0]) for a in range(12, 28)]
    if case == "b":
        return [(a, 0.01, [(125 * j) % NODES for j in range(24)]) for a in range(12, 28)]
    if case == "c":
        return [(12, 0.005 * k, [0]) for k in range(1, 9)]
    raise SystemExit("unknown case " + case)


def run_arm(case, arm, steps, warmup):
    sys.path.insert(0, os.path.join(os.environ.get("GS_TIMING_TREE") or ROOT, "tests"))
    import engine_bind as eb
    gs = eb.gs
    _, st = eb.synth.network(NODES)
    vals = case_values(case)
    origins = [o for _, _, org in vals for o in org]
    if arm == "batched":
        plan = [(dict(trajectories=[(a, p, len(org)) for a, p, org in vals]), origins)]
    elif arm == "single":
        plan = [(dict(active_set_size=max(a for a, _, _ in vals), rotation_probability=vals[-1][1]), origins)]
    else:
        plan = [(dict(active_set_size=a, rotation_probability=p), org) for a, p, org in vals]
    engines = []
    for kw, org in plan:
        e = gs.Engine(st, len(org), fanout=FANOUT, seed=SEED, bfs_mode=gs.GS_BFS_WORKGROUP, **kw)
        e.set_slots(org, 2, 0.15)
        e.init_active_sets()
        engines.append(e)
    total = 0.0
    for e in engines:  # back to back, as a sweep runs its values
        for r in range(warmup):
            e.round(r, record=False)
        e.sync()
        t0 = time.perf_counter()
        for r in range(warmup, warmup + steps):
            e.round(r, record=True)
        e.sync()
        total += time.perf_counter() - t0
    digests = []
    for e in engines:
        summ = e.summaries()
        for k in range(e.n_slots):
            h = hashlib.sha256()
            for x in (e.hops(k), e.pruned_all(k), *e.caches(k), summ[:, k]):
                h.update(x.tobytes())
            digests.append(h.hexdigest()[:16])
    info = engines[0].info()
    print(json.dumps(dict(case=case, arm=arm, engines=len(engines), slots=len(origins), steps=steps,
                          seconds=total, ms_per_round=1e3 * total / steps, fused=info["fused_round"],
                          kernel_hash=gs.lib().gs_kernel_hash().decode(), digests=digests)), flush=True)


def drive(cases, reps, steps, warmup, tree):
    for case in cases:
        runs = {"batched": [], "pervalue": [], "single": []}
        dig = {}
        for rep in range(reps):
            for arm in ("batched", "pervalue") + (("single",) if rep == 0 else ()):
                env = dict(os.environ)
                if arm == "pervalue" and tree:
                    env["GS_TIMING_TREE"] = os.path.abspath(tree)
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", case, "--arm", arm, "--steps",
                                    str(steps), "--warmup", str(warmup)], capture_output=True, text=True, env=env,
                                   timeout=240)
                if r.returncode != 0:  # (nothing more is started on the device after a failed arm)
                    sys.stderr.write(r.stdout + r.stderr)
                    raise SystemExit(f"case {case} arm {arm} exited {r.returncode}")
                out = json.loads(r.stdout.strip().splitlines()[-1])
                runs[arm].append(out["seconds"])
                if arm != "single":
                    dig.setdefault(arm, out["digests"])
                    assert out["digests"] == dig[arm], f"case {case} arm {arm}: digests differ between runs"
        equal = dig["batched"] == dig["pervalue"]
        print(json.dumps(dict(case=case, slots=len(dig["batched"]), steps=steps, pervalue_tree=tree or None,
                              batched_s=runs["batched"], pervalue_s=runs["pervalue"], single_s=runs["single"],
                              every_batched_below_every_pervalue=max(runs["batched"]) < min(runs["pervalue"]),
                              speedup_of_medians=sorted(runs["pervalue"])[len(runs["pervalue"]) // 2] /
                              sorted(runs["batched"])[len(runs["batched"]) // 2],
                              outputs_equal_slot_for_slot=equal)), flush=True)
        if not equal:
            raise SystemExit(f"case {case}: the arms' outputs differ")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--case", default="a", help="a, b, c (with --drive: a comma list)")
    ap.add_argument("--arm", choices=["batched", "pervalue", "single"], default="batched")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--drive", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--pervalue-tree", default="")
    args = ap.parse_args()
    if args.drive:
        drive(args.case.split(","), args.reps, args.steps, args.warmup, args.pervalue_tree)
    else:
        run_arm(args.case, args.arm, args.steps, args.warmup)


if __name__ == "__main__":
    main()
