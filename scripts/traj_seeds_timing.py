#!/usr/bin/env python3
"""Seed replicas as one engine (gs_create_traj_seeds), timed against one engine per seed: 20
warm-up + 100 timed rounds, device-synchronised wall time, fanout 6, bench.py's rotation
probability; seeds SEED, SEED + 1, ...

Shapes: a = C2's network (3,000 synthetic nodes), 64 seeds, origin rank 1, size 12;
        b = C2's network, sizes 12..27 x 4 seeds (64 tables);
        c = 100,000 power-law nodes, 16 seeds, size 12, on the multi-source table engine.

Arms:
  batched   ONE engine of one table per (size, seed)
  perseed   one single-table one-slot engine per (size, seed), back to back; the timed windows
            are summed. Shape c creates, runs and closes each engine in turn (so each may use
            the persistent BFS, which runs only while one engine is alive); shapes a and b
            create all engines first, as a sweep over values does.
  single    one single-table engine of the batched arm's slot count at the largest size and
            the first seed: what the table bank costs per round

One arm per process (`--arm`): prints a JSON line with the timed seconds and a digest per slot
of hops, prune state, caches and recorded summaries. `--drive` runs the arms as child processes,
alternating, `--reps` times each (the single arm once), every child under its own time limit,
ends at the first failure, checks that the batched and per-seed digests agree slot for slot and
prints one summary line per shape. `--perseed-variant NAME` runs the per-seed arm on the library
under gossip-sim_amd/variants/NAME (GS_LIB_VARIANT): a build of the parent commit, so that the
baseline is never the code under test.
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, FANOUT, PROB = 0x5EED0003, 6, 0.013333


def shape_tables(shape):
    """(nodes, multi, [(size, seed)] per table)."""
    if shape == "a":
        return 3000, False, [(12, SEED + k) for k in range(64)]
    if shape == "b":
        return 3000, False, [(a, SEED + k) for a in range(12, 28) for k in range(4)]
    if shape == "c":
        return 100_000, True, [(12, SEED + k) for k in range(16)]
    raise SystemExit("unknown shape " + shape)


def digest(e, k, summ):
    h = hashlib.sha256()
    for x in (e.hops(k), e.pruned_all(k), *e.caches(k), summ[:, k]):
        h.update(x.tobytes())
    return h.hexdigest()[:16]


def run_arm(shape, arm, steps, warmup):
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import engine_bind as eb
    gs = eb.gs
    nodes, multi, tabs = shape_tables(shape)
    if multi:
        st = eb.synth.power_law_stakes(nodes)
    else:
        _, st = eb.synth.network(nodes)
    origin = int(np.argmax(st))  # origin rank 1
    mode = gs.GS_BFS_MULTI if multi else gs.GS_BFS_WORKGROUP
    if arm == "batched":
        plan = [(dict(trajectories=[(a, PROB, 1, sd) for a, sd in tabs], traj_multi=multi), len(tabs))]
    elif arm == "single":
        plan = [(dict(active_set_size=max(a for a, _ in tabs), rotation_probability=PROB, seed=tabs[0][1]), len(tabs))]
    else:
        plan = [(dict(active_set_size=a, rotation_probability=PROB, seed=sd), 1) for a, sd in tabs]

    def create(kw, slots):
        e = gs.Engine(st, slots, fanout=FANOUT, bfs_mode=mode, **kw)
        e.set_slots([origin] * slots, 2, 0.15)
        e.init_active_sets()
        return e

    def timed(e):
        for r in range(warmup):
            e.round(r, record=False)
        e.sync()
        t0 = time.perf_counter()
        for r in range(warmup, warmup + steps):
            e.round(r, record=True)
        e.sync()
        return time.perf_counter() - t0

    total, digests, pers = 0.0, [], []
    engines = [] if multi else [create(kw, slots) for kw, slots in plan]
    for i, (kw, slots) in enumerate(plan):  # back to back, as a sweep runs its values
        e = create(kw, slots) if multi else engines[i]
        total += timed(e)
        summ = e.summaries()
        digests += [digest(e, k, summ) for k in range(slots)]
        pers.append(bool(e.info()["bfs_persistent"]))
        if multi:
            e.close()
    print(json.dumps(dict(shape=shape, arm=arm, engines=len(plan), slots=len(digests), nodes=nodes, steps=steps,
                          seconds=total, ms_per_100_rounds=1e5 * total / steps, persistent_bfs=all(pers),
                          kernel_hash=gs.lib().gs_kernel_hash().decode(), digests=digests)), flush=True)


def drive(shapes, reps, steps, warmup, variant, limit):
    for shape in shapes:
        runs = {"batched": [], "perseed": [], "single": []}
        dig = {}
        for rep in range(reps):
            for arm in ("batched", "perseed") + (("single",) if rep == 0 else ()):
                env = dict(os.environ)
                env.pop("GS_LIB_VARIANT", None)
                if arm == "perseed" and variant:
                    env["GS_LIB_VARIANT"] = variant
                r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__),
                                    "--shape", shape, "--arm", arm, "--steps", str(steps), "--warmup", str(warmup)],
                                   capture_output=True, text=True, env=env)
                if r.returncode != 0:  # (nothing more is started on the device after a failed arm)
                    sys.stderr.write(r.stdout + r.stderr)
                    raise SystemExit(f"shape {shape} arm {arm} exited {r.returncode}")
                out = json.loads(r.stdout.strip().splitlines()[-1])
                print(json.dumps({k: v for k, v in out.items() if k != "digests"}), flush=True)
                runs[arm].append(out["seconds"])
                if arm != "single":
                    dig.setdefault(arm, out["digests"])
                    assert out["digests"] == dig[arm], f"shape {shape} arm {arm}: digests differ between runs"
        equal = dig["batched"] == dig["perseed"]

        def med(x):
            return sorted(x)[len(x) // 2]

        def ms(x):
            return [round(1e5 * s / steps, 3) for s in x]

        print(json.dumps(dict(shape=shape, slots=len(dig["batched"]), steps=steps, perseed_variant=variant or None,
                              batched_ms_per_100_rounds=ms(runs["batched"]), perseed_ms_per_100_rounds=ms(runs["perseed"]),
                              single_ms_per_100_rounds=ms(runs["single"]),
                              every_batched_below_every_perseed=max(runs["batched"]) < min(runs["perseed"]),
                              ratio_of_medians=med(runs["perseed"]) / med(runs["batched"]),
                              table_bank_over_single=med(runs["batched"]) / med(runs["single"]),
                              outputs_equal_slot_for_slot=equal)), flush=True)
        if not equal:
            raise SystemExit(f"shape {shape}: the arms' outputs differ")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shape", default="a", help="a, b, c (with --drive: a comma list)")
    ap.add_argument("--arm", choices=["batched", "perseed", "single"], default="batched")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--drive", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--perseed-variant", default="")
    ap.add_argument("--limit", type=int, default=240, help="seconds per child process (--drive)")
    args = ap.parse_args()
    if args.drive:
        drive(args.shape.split(","), args.reps, args.steps, args.warmup, args.perseed_variant, args.limit)
    else:
        run_arm(args.shape, args.arm, args.steps, args.warmup)


if __name__ == "__main__":
    main()
