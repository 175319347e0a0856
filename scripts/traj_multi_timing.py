#!/usr/bin/env python3
"""BASELINE C3 (100k synthetic power-law nodes, active-set-size sweep 12..27, 16 sims, one
origin each, fanout 6, bench.py's seed and rotation probability; 20 warm-up + 100 timed
rounds with device-synchronised wall time), timed three ways:

  batched    ONE multi-source table engine of 16 one-slot tables (gs_create_traj with
             GS_FLAG_TRAJ_MULTI, bfs_mode GS_BFS_MULTI)
  pervalue   16 single-table one-slot GS_BFS_MULTI engines run back to back: each is created,
             warmed, timed, read and closed before the next (so each may use the persistent BFS,
             which runs only while one engine is alive); the timed windows are summed
  single     one single-table GS_BFS_MULTI engine of 16 slots at size 27: what the table bank
             costs per round

One arm per process (`--arm`): prints a JSON line with the timed seconds and a digest per slot
of hops, prune state, caches and recorded summaries. `--drive` runs the arms as child processes,
alternating, `--reps` times each (the single arm once), every child under its own time limit,
ends at the first failure, checks that the batched and per-value digests agree slot for slot
and prints one summary line. `--pervalue-variant NAME` runs the per-value arm on the library
under gossip-sim_amd/variants/NAME (GS_LIB_VARIANT), e.g. a build of the parent commit.
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, NODES, FANOUT, PROB = 0x5EED0003, 100_000, 6, 0.013333
SIZES = list(range(12, 28))


def digest(e, k, summ):
    h = hashlib.sha256()
    for x in (e.hops(k), e.pruned_all(k), *e.caches(k), summ[:, k]):
        h.update(x.tobytes())
    return h.hexdigest()[:16]


def run_arm(arm, steps, warmup, nodes):
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import engine_bind as eb
    gs = eb.gs
    st = eb.synth.power_law_stakes(nodes)
    origin = int(np.argmax(st))
    if arm == "batched":
        plan = [(dict(trajectories=[(a, PROB, 1) for a in SIZES], traj_multi=True), len(SIZES))]
    elif arm == "single":
        plan = [(dict(active_set_size=max(SIZES), rotation_probability=PROB), len(SIZES))]
    else:
        plan = [(dict(active_set_size=a, rotation_probability=PROB), 1) for a in SIZES]
    total, digests, pers = 0.0, [], []
    for kw, slots in plan:  # back to back, as a sweep runs its values
        e = gs.Engine(st, slots, fanout=FANOUT, seed=SEED, bfs_mode=gs.GS_BFS_MULTI, **kw)
        e.set_slots([origin] * slots, 2, 0.15)
        e.init_active_sets()
        for r in range(warmup):
            e.round(r, record=False)
        e.sync()
        t0 = time.perf_counter()
        for r in range(warmup, warmup + steps):
            e.round(r, record=True)
        e.sync()
        total += time.perf_counter() - t0
        summ = e.summaries()
        digests += [digest(e, k, summ) for k in range(slots)]
        pers.append(bool(e.info()["bfs_persistent"]))
        e.close()
    print(json.dumps(dict(arm=arm, engines=len(plan), slots=len(digests), nodes=nodes, steps=steps, seconds=total,
                          ms_per_round=1e3 * total / steps, persistent_bfs=all(pers),
                          kernel_hash=gs.lib().gs_kernel_hash().decode(), digests=digests)), flush=True)


def drive(reps, steps, warmup, nodes, variant, limit):
    runs = {"batched": [], "pervalue": [], "single": []}
    dig, pers = {}, {}
    for rep in range(reps):
        for arm in ("batched", "pervalue") + (("single",) if rep == 0 else ()):
            env = dict(os.environ)
            env.pop("GS_LIB_VARIANT", None)
            if arm == "pervalue" and variant:
                env["GS_LIB_VARIANT"] = variant
            r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--arm", arm,
                                "--steps", str(steps), "--warmup", str(warmup), "--nodes", str(nodes)],
                               capture_output=True, text=True, env=env)
            if r.returncode != 0:  # (nothing more is started on the device after a failed arm)
                sys.stderr.write(r.stdout + r.stderr)
                raise SystemExit(f"arm {arm} exited {r.returncode}")
            out = json.loads(r.stdout.strip().splitlines()[-1])
            print(json.dumps({k: v for k, v in out.items() if k != "digests"}), flush=True)
            runs[arm].append(out["seconds"])
            pers[arm] = out["persistent_bfs"]
            if arm != "single":
                dig.setdefault(arm, out["digests"])
                assert out["digests"] == dig[arm], f"arm {arm}: digests differ between runs"
    equal = dig["batched"] == dig["pervalue"]

    def med(x):
        return sorted(x)[len(x) // 2]

    print(json.dumps(dict(nodes=nodes, slots=len(dig["batched"]), steps=steps, pervalue_variant=variant or None,
                          batched_s=runs["batched"], pervalue_s=runs["pervalue"], single_s=runs["single"],
                          persistent_bfs=pers,
                          every_batched_below_every_pervalue=max(runs["batched"]) < min(runs["pervalue"]),
                          speedup_of_medians=med(runs["pervalue"]) / med(runs["batched"]),
                          outputs_equal_slot_for_slot=equal)), flush=True)
    if not equal:
        raise SystemExit("the arms' outputs differ")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--arm", choices=["batched", "pervalue", "single"], default="batched")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--nodes", type=int, default=NODES)
    ap.add_argument("--drive", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--pervalue-variant", default="")
    ap.add_argument("--limit", type=int, default=240, help="seconds per child process (--drive)")
    args = ap.parse_args()
    if args.drive:
        drive(args.reps, args.steps, args.warmup, args.nodes, args.pervalue_variant, args.limit)
    else:
        run_arm(args.arm, args.steps, args.warmup, args.nodes)


if __name__ == "__main__":
    main()
