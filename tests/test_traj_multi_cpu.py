"""Trajectory tables on the multi-source BFS, without a GPU: gs_traj_multi_supported against
the multi BFS's geometry rule, the batched sweep's multi rule, the CLI's --batch-sweeps
--bfs-mode 4 engine plan from a replayed run, the new symbols, and the host-side group-table
builder (csrc/gs_mv_groups.h) through a stand-alone C++ program built with the host compiler's
address and undefined-behaviour sanitizers."""
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
LDS = 160 * 1024
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _clog2(x):
    l = 0
    while (1 << l) < x:
        l += 1
    return l


def mv_rule(n, slots, fanout, asz):
    """mv_geometry + mv_supported + the 2^32 area bound of gs_bfs_multi.hip / gs_engine.hip for an
    engine of several tables (a node takes up to min(group slots, 28) frontier entries per level).
    Returns (supported, group width, area records)."""
    if n < 2 or n > 2**24 - 1 or slots < 1 or fanout < 1 or not 1 <= asz <= 32 or n * slots >= 2**32:
        return False, 0, 0
    aszp = (asz + 3) & ~3
    ub = max(1, _clog2(n))
    bsc = min(13, max(6, ub - 8 if ub > 8 else 0))
    bsf = max(min(bsc, 9), bsc - 4 if bsc > 4 else 0)
    nbc = (n + (1 << bsc) - 1) >> bsc
    gw = min(28, (64 - ub - bsc) & ~3, (64 - ub - bsf - 8) & ~3)
    hist = 4 * ((nbc + 17 + 1) & ~1)
    xt = 1024 if nbc >= 512 and hist + 1024 * aszp * 8 <= LDS else 256
    q_cap = n * min(slots, gw, 28) + 64
    rows = (q_cap + xt - 1) // xt + 1
    area = rows * xt * asz
    apply_lds = 4 * (2 * 1024 + 1 + 2 * (1 << bsc) + 64 + 96)
    ok = hist + xt * aszp * 8 <= LDS and apply_lds <= LDS and gw >= 4 and area <= 0xFFFFFFF0
    return ok, gw, area


def test_traj_multi_supported_follows_the_geometry_rule():
    """The C function against the rule, at sizes on both sides of the workgroup engine's limit, at
    the largest network, and at one refused by the area bound alone. The rule's group-width term
    (GW >= 4) cannot refuse a valid node count: GW is at least 20 up to 2^24 - 1 nodes, which the
    loop below establishes, so no refusal by it can be constructed through this interface."""
    cases = [(2, 1, 1, 1), (60, 3, 6, 16), (260, 32, 6, 27), (400, 28, 6, 32), (17000, 2, 6, 13), (20000, 6, 6, 27),
             (70000, 2, 6, 12), (100000, 16, 6, 27), (10**6, 28, 6, 32), (2**24 - 1, 2, 6, 12), (2**24 - 1, 28, 6, 32),
             (2**24 - 1, 28, 6, 8), (2**23, 64, 12, 20)]
    for c in cases:
        assert gs.traj_multi_supported(*c) == mv_rule(*c)[0], c
    assert gs.traj_multi_supported(100000, 16, 6, 27)       # C3: sizes 12..27, 16 sims
    assert not gs.traj_supported(100000, 6, 27)[0]
    # refused by the area bound alone: the same network and slots fit at a smaller capacity
    ok, gw, area = mv_rule(2**24 - 1, 28, 6, 32)
    assert not ok and gw >= 4 and area > 0xFFFFFFF0
    assert not gs.traj_multi_supported(2**24 - 1, 28, 6, 32) and gs.traj_multi_supported(2**24 - 1, 28, 6, 8)
    assert min(mv_rule(1 << b, 28, 6, 12)[1] for b in range(1, 24)) >= 20 and mv_rule(2**24 - 1, 28, 6, 12)[1] == 20
    for bad in [(1, 2, 6, 12), (2**24, 2, 6, 12), (100, 0, 6, 12), (100, 2, 0, 12), (100, 2, 6, 0), (100, 2, 6, 33),
                (2**24 - 1, 257, 6, 12)]:
        assert not gs.traj_multi_supported(*bad), bad


def test_traj_batchable_multi():
    def cfgs(sizes, **kw):
        return [dict(asz=a, seed=3, **kw) for a in sizes]

    assert sw.traj_batchable_multi(cfgs([12, 20, 27]), 100000) and not sw.traj_batchable(cfgs([12, 20, 27]), 100000)
    assert sw.traj_batchable_multi(cfgs([12, 20]), 150) and sw.traj_batchable(cfgs([12, 20]), 150)
    assert not sw.traj_batchable_multi([], 150)
    assert not sw.traj_batchable_multi([dict(asz=12, seed=1), dict(asz=13, seed=2)], 150)     # seeds differ
    assert not sw.traj_batchable_multi([dict(asz=12, n_sims=2), dict(asz=13, n_sims=2)], 150)
    assert not sw.traj_batchable_multi(cfgs([12, 40]), 150)                                    # size above 32
    assert not sw.traj_batchable_multi(cfgs([32] * 28), 2**24 - 1)                             # the area bound


def test_run_traj_sweep_multi_plan_with_a_stub_runner():
    """multi=True: a share beyond the workgroup engine runs as ONE engine with bfs_mode GS_BFS_MULTI;
    a share that fits the workgroup engine runs as before; multi=False changes nothing."""
    calls = []

    class Res:
        def __init__(self, vals):
            self.vals = vals

        def f64(self, j, name):
            return np.array([float(self.vals[j])])

        def u64(self, j, name):
            return np.array([self.vals[j]], dtype=np.uint64)

    def runner(stakes, *, n_sims, **kw):
        calls.append((n_sims, kw.get("aszs"), kw.get("bfs_mode"), kw.get("asz")))
        return Res(kw["aszs"] if "aszs" in kw else [kw["asz"]])

    sizes = [6, 12, 18]
    out = sw.run_traj_sweep(np.zeros(70000), sizes, lambda a: dict(asz=a, seed=3), runner=runner, multi=True)
    assert calls == [(3, sizes, gs.GS_BFS_MULTI, None)]
    assert [int(out.u64(i, "origin")[0]) for i in range(3)] == sizes
    del calls[:]
    sw.run_traj_sweep(np.zeros(70000), sizes, lambda a: dict(asz=a, seed=3), runner=runner)
    assert calls == [(1, None, None, a) for a in sizes]
    del calls[:]
    sw.run_traj_sweep(np.zeros(150), sizes, lambda a: dict(asz=a, seed=3), runner=runner, multi=True)
    assert calls == [(3, sizes, None, None)]  # fits the workgroup engine: that engine, as before
    del calls[:]
    sw.run_traj_sweep(np.zeros(70000), sizes, lambda a: dict(asz=a, seed=a), runner=runner, multi=True)  # seeds differ
    assert [c[0] for c in calls] == [1, 1, 1]


def test_cli_engine_plan_at_17000_nodes(tmp_path):
    """--batch-sweeps --bfs-mode 4 plans one multi-source table engine where the default mode
    still falls back to one engine per value (with its log line)."""
    plan, res = str(tmp_path / "plan.txt"), str(tmp_path / "r.txt")
    rr.write_results(res, [({}, {})] * 2)
    base = ["--synthetic", 17000, "--iterations", 5, "--warm-up-rounds", 5, "--replay-results", res, "--engine-plan",
            plan, "--num-simulations", 2, "--origin-rank", 1, 1, 1, "--test-type", "active-set-size", "--batch-sweeps"]
    p0 = float(".013333")
    r = cli(*base, "--bfs-mode", 4)
    assert open(plan).read().splitlines() == [
        "device 0 sims 0,1 active-set-size 12,13 fanouts 6,6 rotation-probability %.17g,%.17g" % (p0, p0)]
    assert not any("one engine per value" in ln for ln in r.stderr.splitlines())
    r = cli(*base)
    assert open(plan).read().splitlines() == [f"device 0 sims {i} active-set-size {12 + i} fanouts 6" for i in range(2)]
    assert sum("--batch-sweeps" in ln and "one engine per value" in ln for ln in r.stderr.splitlines()) == 1
    # without --batch-sweeps the mode alone plans nothing new
    cli(*[a for a in base if a != "--batch-sweeps"], "--bfs-mode", 4)
    assert open(plan).read().splitlines() == [f"device 0 sims {i} active-set-size {12 + i} fanouts 6" for i in range(2)]


def test_cli_help_documents_the_multi_table_engine():
    h = cli("--help").stdout
    assert "--batch-sweeps" in h and "--bfs-mode 4" in h


def test_new_symbols_are_declared_exported_and_bound():
    assert "gs_traj_multi_supported" in set(declared_symbols()) and "gs_traj_multi_supported" in gs.EXPORTS
    assert hasattr(gs.lib(), "gs_traj_multi_supported")
    assert gs.GS_FLAG_TRAJ_MULTI == 256
    hdr = open(os.path.join(ROOT, "include", "gossip_hip.h")).read()
    assert "GS_FLAG_TRAJ_MULTI = 256" in hdr
    import inspect
    assert "traj_multi" in inspect.signature(gs.Engine.__init__).parameters
    assert "multi" in inspect.signature(sw.run_traj_sweep).parameters


def test_group_table_builder_under_host_sanitizers(tmp_path):
    """tests/mv_groups_check.cpp: for a hand-made slot / table layout the table masks partition each
    group's slots, the seeds are per (origin, table), and a straddling table appears in both
    groups. A stand-alone program with its own main, compiled with -fsanitize=address,undefined
    on the host compiler and run directly."""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "mv_groups_check")
    # (the sanitizer runtimes linked statically: the program needs nothing loaded before it)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan",
                    "-static-libubsan", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "gossip-sim_amd", "csrc"),
                    os.path.join(ROOT, "tests", "mv_groups_check.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr
