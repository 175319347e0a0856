"""A Philox seed per trajectory table, without a GPU: the new symbols, the trial sweep's batching
rules and plan (stub runner), the CLI's --trials engine plan from a replayed run, and the
grouping header under the host sanitizers."""
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

import engine_bind as eb
import gossip_sim_amd.sweep as sw
import report_ref as rr
from test_abi import declared_symbols
from test_cli import cli, yaml_net  # noqa: F401

gs = eb.gs
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def test_new_symbols_are_declared_exported_and_bound():
    new = {"gs_create_traj_seeds", "gs_engine_traj_seeds", "gs_run_simulations_seeds"}
    assert new <= set(declared_symbols()) and new <= set(gs.EXPORTS)
    lib = gs.lib()
    assert all(hasattr(lib, s) for s in new)
    assert "seeds" in inspect.signature(gs.run_simulations).parameters
    assert hasattr(gs.Engine, "table_seeds")
    for f in (sw.trial_batchable, sw.trial_batchable_multi, sw.run_trial_sweep):
        assert callable(f)
    assert "multi" in inspect.signature(sw.run_trial_sweep).parameters


def test_mixed_tuples_raise_before_any_engine():
    st = np.full(50, 10**9, dtype=np.uint64)
    for tr in ([(12, .1, 1, 5), (8, .1, 2)], [(12, .1, 1), (8, .1, 2, 5)], [(12, .1)], [(12, .1, 1, 2, 3)]):
        with pytest.raises(ValueError):
            gs.Engine(st, 3, trajectories=tr)
    with pytest.raises(ValueError):
        gs.run_simulations(st, n_sims=3, seeds=[1, 2])


def test_trial_batchable_rules():
    base = dict(asz=12, p=.05, fanout=6, iterations=30, warm_up=5)
    seeds = [dict(base, seed=s) for s in (1, 2, 3)]
    assert sw.trial_batchable(seeds, 3000) and not sw.traj_batchable(seeds, 3000)  # (seeds differ: only as trials)
    both = [dict(base, seed=s, asz=a) for a in (8, 12) for s in (1, 2)]
    assert sw.trial_batchable(both, 3000)
    assert sw.trial_batchable([dict(base, seed=1), dict(base)], 3000)  # (a missing seed is a seed too)
    assert not sw.trial_batchable([], 3000)
    assert not sw.trial_batchable([dict(base, seed=1), dict(base, seed=2, iterations=31)], 3000)  # more than the keys
    assert not sw.trial_batchable([dict(base, seed=1), dict(base, seed=2, n_sims=2)], 3000)
    assert not sw.trial_batchable([dict(base, seed=1, origin_ranks=[1]), dict(base, seed=2)], 3000)
    # the network rules are traj_batchable's: seeds do not enter the geometry
    assert not sw.trial_batchable(seeds, 70000) and sw.trial_batchable_multi(seeds, 70000)
    assert not sw.trial_batchable_multi([dict(base, seed=1), dict(base, seed=2, iterations=31)], 70000)
    same = [dict(base, seed=4, asz=a) for a in (8, 12)]
    assert sw.trial_batchable(same, 3000) == sw.traj_batchable(same, 3000) is True


class _Res:
    def __init__(self, vals):
        self.vals = vals

    def f64(self, j, name):
        return np.array([float(self.vals[j])])

    def u64(self, j, name):
        return np.array([self.vals[j]], dtype=np.uint64)


def _stub(calls):
    def runner(stakes, *, n_sims, **kw):
        calls.append(dict(kw, n_sims=n_sims))
        if "seeds" in kw:  # a sim's stand-in result: 1000 * size + seed
            return _Res([1000 * a + s for a, s in zip(kw["aszs"], kw["seeds"])])
        return _Res([1000 * kw.get("asz", 12) + kw["seed"]])
    return runner


def test_run_trial_sweep_plan_with_a_stub_runner():
    calls = []
    sizes, seeds = [6, 12, 18], [7, 8]
    want = [1000 * a + s for a in sizes for s in seeds]  # value-major: index i_value * len(seeds) + i_seed
    out = sw.run_trial_sweep(np.zeros(150), sizes, seeds, lambda a: dict(asz=a, p=.25, fanout=5, seed=99),
                             runner=_stub(calls))
    assert len(calls) == 1 and calls[0]["n_sims"] == 6
    assert calls[0]["seeds"] == [7, 8, 7, 8, 7, 8] and calls[0]["aszs"] == [6, 6, 12, 12, 18, 18]
    assert calls[0]["rot_probs"] == [.25] * 6 and calls[0]["fanouts"] == [5] * 6
    assert "seed" not in calls[0] and "asz" not in calls[0] and "bfs_mode" not in calls[0]
    assert out.n_sims == 6 and [int(out.u64(i, "origin")[0]) for i in range(6)] == want
    # plain replicas: values=[None]
    del calls[:]
    out = sw.run_trial_sweep(np.zeros(150), [None], [3, 4, 5], lambda _: dict(asz=12, origin_ranks=[2]),
                             runner=_stub(calls))
    assert len(calls) == 1 and calls[0]["seeds"] == [3, 4, 5] and calls[0]["origin_ranks"] == [2, 2, 2]
    assert [int(out.u64(i, "origin")[0]) for i in range(3)] == [12003, 12004, 12005]
    # above the workgroup limit: one engine per unit, each at its own seed
    del calls[:]
    out = sw.run_trial_sweep(np.zeros(70000), sizes, seeds, lambda a: dict(asz=a), runner=_stub(calls))
    assert [(c["n_sims"], c["asz"], c["seed"]) for c in calls] == [(1, a, s) for a in sizes for s in seeds]
    assert all("seeds" not in c for c in calls)
    assert [int(out.u64(i, "origin")[0]) for i in range(6)] == want
    # ... unless multi=True: one multi-source table engine
    del calls[:]
    out = sw.run_trial_sweep(np.zeros(70000), sizes, seeds, lambda a: dict(asz=a), runner=_stub(calls), multi=True)
    assert len(calls) == 1 and calls[0]["bfs_mode"] == gs.GS_BFS_MULTI and calls[0]["seeds"] == [7, 8] * 3
    assert [int(out.u64(i, "origin")[0]) for i in range(6)] == want
    # multi=True where the workgroup engine fits changes nothing
    del calls[:]
    sw.run_trial_sweep(np.zeros(150), sizes, seeds, lambda a: dict(asz=a), runner=_stub(calls), multi=True)
    assert len(calls) == 1 and "bfs_mode" not in calls[0]
    # kwargs that differ in more than the table keys: per unit
    del calls[:]
    sw.run_trial_sweep(np.zeros(150), sizes, seeds, lambda a: dict(asz=a, iterations=a), runner=_stub(calls))
    assert [c["n_sims"] for c in calls] == [1] * 6
    # one unit is one plain engine
    del calls[:]
    sw.run_trial_sweep(np.zeros(150), [12], [9], lambda a: dict(asz=a), runner=_stub(calls))
    assert [(c["n_sims"], c["seed"]) for c in calls] == [(1, 9)]
    # run_traj_sweep keeps refusing seeds that differ
    del calls[:]
    sw.run_traj_sweep(np.zeros(150), sizes, lambda a: dict(asz=a, seed=a), runner=_stub(calls))
    assert [c["n_sims"] for c in calls] == [1, 1, 1]


def _plan(yaml_net, tmp_path, *extra, n=3, k=1):
    path = yaml_net[0]
    plan, res = str(tmp_path / "plan.txt"), str(tmp_path / "r.txt")
    rr.write_results(res, [({}, {})] * (n * k))
    r = cli("--accounts-from-yaml", "--account-file", path, "--iterations", 5, "--warm-up-rounds", 5,
            "--replay-results", res, "--engine-plan", plan, "--num-simulations", n, "--origin-rank", *([1] * (n + 1)),
            *extra)
    return open(plan).read().splitlines(), r


def test_cli_trials_plan_with_replay(yaml_net, tmp_path):
    p0 = float(".013333")
    size = ["--test-type", "active-set-size", "--step-size", 2]
    ingress = ["--test-type", "min-ingress-nodes"]
    seed = ["--seed", 100]
    # K = 1: byte-identical to the lines without the flag
    for extra in (size, size + ["--batch-sweeps"], ingress, size + ["--batch-sweeps", "--gpus", 2]):
        a = _plan(yaml_net, tmp_path, *extra, *seed)[0]
        assert a == _plan(yaml_net, tmp_path, *extra, *seed, "--trials", 1)[0] and all("seeds" not in ln for ln in a)
    assert _plan(yaml_net, tmp_path, *size, *seed)[0] == [f"device 0 sims {i} active-set-size {12 + 2 * i} fanouts 6"
                                                          for i in range(3)]
    # K = 2 without --batch-sweeps: today's plan once per seed (value-major, trial-minor simulations)
    assert _plan(yaml_net, tmp_path, *size, *seed, "--trials", 2, k=2)[0] == [
        f"device 0 sims {2 * i + k} active-set-size {12 + 2 * i} fanouts 6 seeds {100 + k}"
        for i in range(3) for k in range(2)]
    assert _plan(yaml_net, tmp_path, *ingress, *seed, "--trials", 2, k=2)[0] == [
        "device 0 sims 0,2,4 active-set-size 12 fanouts 6,6,6 seeds 100",
        "device 0 sims 1,3,5 active-set-size 12 fanouts 6,6,6 seeds 101"]
    assert _plan(yaml_net, tmp_path, *size, *seed, "--trials", 2, "--gpus", 2, k=2)[0] == [
        f"device {k} sims {2 * i + k} active-set-size {12 + 2 * i} fanouts 6 seeds {100 + k}"
        for i in range(3) for k in range(2)]
    # with --batch-sweeps: one engine per device, a table per (value, seed)
    probs6 = ",".join("%.17g" % p0 for _ in range(6))
    assert _plan(yaml_net, tmp_path, *size, *seed, "--trials", 2, "--batch-sweeps", k=2)[0] == [
        "device 0 sims 0,1,2,3,4,5 active-set-size 12,12,14,14,16,16 fanouts 6,6,6,6,6,6 rotation-probability " +
        probs6 + " seeds 100,101,100,101,100,101"]
    probs3 = ",".join("%.17g" % p0 for _ in range(3))
    assert _plan(yaml_net, tmp_path, *size, *seed, "--trials", 2, "--batch-sweeps", "--gpus", 2, k=2)[0] == [
        "device 0 sims 0,1,2 active-set-size 12,12,14 fanouts 6,6,6 rotation-probability " + probs3 +
        " seeds 100,101,100",
        "device 1 sims 3,4,5 active-set-size 14,16,16 fanouts 6,6,6 rotation-probability " + probs3 +
        " seeds 101,100,101"]
    # plain replicas (no test type) batch as well: the seeds are the tables
    assert _plan(yaml_net, tmp_path, *seed, "--trials", 3, "--batch-sweeps", n=1, k=3)[0] == [
        "device 0 sims 0,1,2 active-set-size 12,12,12 fanouts 6,6,6 rotation-probability " + probs3 +
        " seeds 100,101,102"]
    assert _plan(yaml_net, tmp_path, *seed, "--trials", 3, n=1, k=3)[0] == [
        f"device 0 sims {k} active-set-size 12 fanouts 6 seeds {100 + k}" for k in range(3)]
    # the replayed file must hold every repeat
    path = yaml_net[0]
    res = str(tmp_path / "short.txt")
    rr.write_results(res, [({}, {})] * 3)
    r = cli("--accounts-from-yaml", "--account-file", path, "--iterations", 5, "--warm-up-rounds", 5,
            "--replay-results", res, "--num-simulations", 3, "--origin-rank", 1, 1, 1, 1, "--trials", 2, check=False)
    assert r.returncode == 1 and "holds 3 simulations, not 6" in r.stderr
    assert cli("--synthetic", 20, "--trials", 0, check=False).returncode == 2


def test_cli_trials_falls_back_when_the_network_does_not_fit(tmp_path):
    plan, res = str(tmp_path / "plan.txt"), str(tmp_path / "r.txt")
    rr.write_results(res, [({}, {})] * 4)
    args = ["--synthetic", 17000, "--iterations", 5, "--warm-up-rounds", 5, "--replay-results", res, "--engine-plan",
            plan, "--num-simulations", 2, "--origin-rank", 1, 1, 1, "--test-type", "active-set-size", "--batch-sweeps",
            "--trials", 2, "--seed", 5]
    r = cli(*args)
    assert open(plan).read().splitlines() == [f"device 0 sims {2 * i + k} active-set-size {12 + i} fanouts 6 seeds {5 + k}"
                                              for i in range(2) for k in range(2)]
    assert sum("--batch-sweeps" in ln and "one engine per value" in ln for ln in r.stderr.splitlines()) == 1
    cli(*args, "--bfs-mode", 4)  # the multi-source table engine holds it
    assert open(plan).read().splitlines() == [
        "device 0 sims 0,1,2,3 active-set-size 12,12,13,13 fanouts 6,6,6,6 rotation-probability " +
        ",".join("%.17g" % float(".013333") for _ in range(4)) + " seeds 5,6,5,6"]


def test_cli_help_lists_trials():
    assert "--trials" in cli("--help").stdout


def test_grouping_header_under_host_sanitizers(tmp_path):
    """tests/traj_plan_check.cpp: non-adjacent equal triples merge, tables stand in first-occurrence
    order, the permutation and its inverse, one triple collapses, NULL columns fall back to the
    configuration's values. A stand-alone program with its own main, compiled with
    -fsanitize=address,undefined on the host compiler and run directly."""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "traj_plan_check")
    # (the sanitizer runtimes linked statically: the program needs nothing loaded before it)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan",
                    "-static-libubsan", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "gossip-sim_amd", "csrc"),
                    os.path.join(ROOT, "tests", "traj_plan_check.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr
