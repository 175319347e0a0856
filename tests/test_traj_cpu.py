"""Trajectory tables without a GPU: gs_traj_supported against the workgroup engine's LDS
rule, the batched sweep's table grouping and dealing, the CLI's --batch-sweeps engine plan
from a replayed run, and the header's new symbols."""
import numpy as np

import engine_bind as eb
import gossip_sim_amd.sweep as sw
import report_ref as rr
from test_abi import declared_symbols
from test_cli import cli, yaml_net  # noqa: F401

gs = eb.gs
LDS = 160 * 1024


def _a4(x):
    return (x + 3) & ~3


def bfs_lds(n):
    """k_bfs_wg: control words, hop histogram, u32 in-degrees, hops, egress, two u16 queues."""
    return 64 + 1024 + 4 * n + 2 * _a4(n) + 2 * 2 * ((n + 1) & ~1)


def round_lds(n, fanout, asz):
    """k_round_wg (768 threads): control, histogram, per-wave scratch, u16 in-degrees, queue /
    segment offsets, push masks, prune masks, egress, ring head/len, hops, stranded bitmap, records."""
    fcap, aszp = min(fanout, asz), _a4(asz)
    pmw, offw = (2 if aszp <= 16 else 4), (2 if fcap * n <= 0xFFFF else 4)
    return (32 * 4 + 256 * 4 + 12 * 128 * 4 + 4 * ((n + 1) // 2) + _a4(offw * n) + 2 * _a4(pmw * n) + _a4(n) +
            _a4(2 * n) + _a4(n) + 4 * ((n + 31) // 32) + _a4(2 * fcap * n))


def test_traj_supported_follows_the_lds_rule():
    assert gs.traj_supported(3000, 6, 27) == (True, True)    # the headline network, sizes 12..27
    assert gs.traj_supported(3000, 6, 12) == (True, True)
    edge = max(n for n in range(16000, 16400) if bfs_lds(n) <= LDS)
    for n, f, a in [(2, 1, 1), (240, 6, 20), (3000, 32, 32), (5000, 6, 12), (5000, 12, 12), (8000, 6, 32),
                    (9000, 6, 12), (edge, 6, 12), (edge + 1, 6, 12), (16384, 6, 12), (65535, 6, 12), (65536, 6, 12)]:
        ok = n <= 65535 and bfs_lds(n) <= LDS
        assert gs.traj_supported(n, f, a) == (ok, ok and round_lds(n, f, a) <= LDS), (n, f, a)
    assert gs.traj_supported(edge, 6, 12)[0] and not gs.traj_supported(edge + 1, 6, 12)[0]
    assert gs.traj_supported(8000, 6, 32) == (True, False)   # step kernels only: the round's layout is too large
    for bad in [(1, 6, 12), (100, 0, 12), (100, 6, 0), (100, 6, 33)]:
        assert gs.traj_supported(*bad) == (False, False)


def test_traj_tables_and_units():
    assert sw.traj_tables([6, 12, 18], [.1, .1, .1]) == [(6, .1, [0]), (12, .1, [1]), (18, .1, [2])]
    assert sw.traj_tables([12, 12, 12], [.1, .2, .1]) == [(12, .1, [0, 2]), (12, .2, [1])]  # equal pairs not adjacent
    assert sw.traj_tables([8, 12, 8, 12], [.5] * 4) == [(8, .5, [0, 2]), (12, .5, [1, 3])]
    assert sw.traj_tables([], []) == []
    assert sw.traj_units(5, 1) == [(0, [0, 1, 2, 3, 4])]
    assert sw.traj_units(5, 2) == [(0, [0, 2, 4]), (1, [1, 3])]    # dealt round-robin, as run_sweep deals
    assert sw.traj_units(2, 4) == [(0, [0]), (1, [1])]
    for world in range(1, 7):
        units = sw.traj_units(11, world)
        assert sorted(i for _, u in units for i in u) == list(range(11))
        assert all(u == sw.shard(11, r, world) for r, u in units)


def test_run_traj_sweep_plan_with_a_stub_runner():
    """A share that fits runs as one engine with per-sim sizes, probabilities and fanouts; one
    that does not (too many nodes, or kwargs that differ in more) runs one engine per value."""
    calls = []

    class Res:
        def __init__(self, vals):
            self.vals = vals

        def f64(self, j, name):
            return np.array([float(self.vals[j])])

        def u64(self, j, name):
            return np.array([self.vals[j]], dtype=np.uint64)

    def runner(stakes, *, n_sims, **kw):
        calls.append((n_sims, kw.get("aszs"), kw.get("rot_probs"), kw.get("fanouts"), kw.get("asz"), kw["seed"]))
        return Res(kw["aszs"] if "aszs" in kw else [kw["asz"]])

    sizes = [6, 12, 18]
    out = sw.run_traj_sweep(np.zeros(150), sizes, lambda a: dict(asz=a, p=.25, fanout=5, seed=3), runner=runner)
    assert calls == [(3, [6, 12, 18], [.25] * 3, [5] * 3, None, 3)]
    assert [int(out.u64(i, "origin")[0]) for i in range(3)] == sizes
    del calls[:]
    out = sw.run_traj_sweep(np.zeros(70000), sizes, lambda a: dict(asz=a, seed=3), runner=runner)
    assert calls == [(1, None, None, None, a, 3) for a in sizes]
    assert [int(out.u64(i, "origin")[0]) for i in range(3)] == sizes
    del calls[:]
    sw.run_traj_sweep(np.zeros(150), sizes, lambda a: dict(asz=a, seed=a), runner=runner)  # seeds differ
    assert [c[0] for c in calls] == [1, 1, 1]


def _plan(yaml_net, tmp_path, *extra, n=3):
    path = yaml_net[0]
    plan, res = str(tmp_path / "plan.txt"), str(tmp_path / "r.txt")
    rr.write_results(res, [({}, {})] * n)
    r = cli("--accounts-from-yaml", "--account-file", path, "--iterations", 5, "--warm-up-rounds", 5,
            "--replay-results", res, "--engine-plan", plan, "--num-simulations", n, "--origin-rank", *([1] * (n + 1)),
            *extra)
    return open(plan).read().splitlines(), r


def test_cli_batch_sweeps_plan_with_replay(yaml_net, tmp_path):
    p0 = float(".013333")
    size = ["--test-type", "active-set-size", "--step-size", 2]
    rot = ["--test-type", "rotate-probability", "--step-size", 0.25]
    fan = ["--test-type", "push-fanout", "--push-fanout", 2, "--step-size", 3]
    probs3 = ",".join("%.17g" % p0 for _ in range(3))
    # without the flag: the parent's lines
    assert _plan(yaml_net, tmp_path, *size)[0] == [f"device 0 sims {i} active-set-size {12 + 2 * i} fanouts 6"
                                                   for i in range(3)]
    assert _plan(yaml_net, tmp_path, *rot)[0] == [f"device 0 sims {i} active-set-size 12 fanouts 6" for i in range(3)]
    assert _plan(yaml_net, tmp_path, *fan, n=5)[0] == ["device 0 sims 0,1,2,3 active-set-size 12 fanouts 2,5,8,11",
                                                       "device 0 sims 4 active-set-size 14 fanouts 14"]
    # with it: one line of per-sim lists
    assert _plan(yaml_net, tmp_path, *size, "--batch-sweeps")[0] == [
        "device 0 sims 0,1,2 active-set-size 12,14,16 fanouts 6,6,6 rotation-probability " + probs3]
    assert _plan(yaml_net, tmp_path, *rot, "--batch-sweeps")[0] == [
        "device 0 sims 0,1,2 active-set-size 12,12,12 fanouts 6,6,6 rotation-probability " +
        ",".join("%.17g" % (p0 + i * 0.25) for i in range(3))]
    assert _plan(yaml_net, tmp_path, *fan, "--batch-sweeps", n=5)[0] == [
        "device 0 sims 0,1,2,3,4 active-set-size 12,12,12,12,14 fanouts 2,5,8,11,14 rotation-probability " +
        ",".join("%.17g" % p0 for _ in range(5))]
    # ... split into contiguous chunks over --gpus
    assert _plan(yaml_net, tmp_path, *size, "--batch-sweeps", "--gpus", 2)[0] == [
        "device 0 sims 0 active-set-size 12 fanouts 6 rotation-probability %.17g" % p0,
        "device 1 sims 1,2 active-set-size 14,16 fanouts 6,6 rotation-probability %.17g,%.17g" % (p0, p0)]
    # the other sweeps are unchanged by the flag
    ranks = ["--test-type", "min-ingress-nodes"]
    assert _plan(yaml_net, tmp_path, *ranks, "--batch-sweeps")[0] == _plan(yaml_net, tmp_path, *ranks)[0] == [
        "device 0 sims 0,1,2 active-set-size 12 fanouts 6,6,6"]


def test_cli_batch_sweeps_falls_back_when_the_network_does_not_fit(tmp_path):
    plan, res = str(tmp_path / "plan.txt"), str(tmp_path / "r.txt")
    rr.write_results(res, [({}, {})] * 2)
    r = cli("--synthetic", 17000, "--iterations", 5, "--warm-up-rounds", 5, "--replay-results", res, "--engine-plan",
            plan, "--num-simulations", 2, "--origin-rank", 1, 1, 1, "--test-type", "active-set-size", "--batch-sweeps")
    assert open(plan).read().splitlines() == [f"device 0 sims {i} active-set-size {12 + i} fanouts 6" for i in range(2)]
    assert sum("--batch-sweeps" in ln and "one engine per value" in ln for ln in r.stderr.splitlines()) == 1


def test_cli_help_lists_batch_sweeps():
    assert "--batch-sweeps" in cli("--help").stdout


def test_new_symbols_are_declared_and_bound():
    new = {"gs_create_traj", "gs_engine_traj", "gs_traj_supported", "gs_set_active_set_entry_traj",
           "gs_get_active_set_entry_traj", "gs_read_active_sets_traj", "gs_run_simulations_traj"}
    assert new <= set(declared_symbols()) and new <= set(gs.EXPORTS)
    lib = gs.lib()
    assert all(hasattr(lib, s) for s in new)
