"""The push-fanout sweep's engine plan without a GPU: sweep.fanout_groups / fanout_units,
and the CLI's --engine-plan written from a replayed run."""
import numpy as np

import engine_bind as eb  # noqa: F401  (makes gossip_sim_amd importable)
import gossip_sim_amd.sweep as sw
import report_ref as rr
from test_cli import cli, oracle_sims, sweep_params, yaml_net  # noqa: F401


def test_fanout_groups():
    assert sw.fanout_groups([2, 5, 8, 11, 14], 12) == [[0, 1, 2, 3], [4]]
    assert sw.fanout_groups([1, 2, 3, 6, 9, 12], 12) == [[0, 1, 2, 3, 4, 5]]   # case A: one engine
    assert sw.fanout_groups([1, 7, 20, 32], 32) == [[0, 1, 2, 3]]             # case C
    assert sw.fanout_groups([1, 3, 7], 7) == [[0, 1, 2]]                      # case D
    assert sw.fanout_groups([1 + k % 12 for k in range(36)], 12) == [list(range(36))]  # case E
    # every value above the active-set size raises it: one group each ...
    assert sw.fanout_groups([13, 14, 15], 12) == [[0], [1], [2]]
    # ... unless the values are equal
    assert sw.fanout_groups([13, 14, 13, 14], 12) == [[0, 2], [1, 3]]
    # sim order inside a group, groups in order of their first sim
    assert sw.fanout_groups([14, 2, 13, 5, 14, 12], 12) == [[0, 4], [1, 3, 5], [2]]
    assert sw.fanout_groups([], 12) == []


def test_fanout_units_over_ranks():
    f = [2, 5, 8, 11, 14]
    assert sw.fanout_units(f, 12, 1) == [(0, [0, 1, 2, 3]), (0, [4])]
    assert sw.fanout_units(f, 12, 2) == [(0, [0, 1, 2, 3]), (1, [4])]           # as many groups as ranks: dealt
    assert sw.fanout_units(f, 12, 3) == [(0, [0, 1]), (1, [2, 3]), (2, [4])]    # fewer: the largest group is split
    assert sw.fanout_units([2, 3], 12, 4) == [(0, [0]), (1, [1])]               # single sims are not split
    # every sim exactly once, whatever the world size
    for world in range(1, 8):
        units = sw.fanout_units([1 + k % 14 for k in range(20)], 12, world)
        assert sorted(i for _, u in units for i in u) == list(range(20))
        assert all(0 <= r < world for r, _ in units)


def test_run_fanout_sweep_plan_with_a_stub_runner():
    """run_fanout_sweep hands each group to the runner as one engine: n_sims, the per-sim
    fanouts, the capacity and the raised active-set size."""
    calls = []

    class Res:
        def __init__(self, fanouts):
            self.fanouts = fanouts

        def f64(self, j, name):
            return np.array([float(self.fanouts[j])])

        def u64(self, j, name):
            return np.array([self.fanouts[j]], dtype=np.uint64)

    def runner(stakes, *, n_sims, fanouts, **kw):
        calls.append((n_sims, list(fanouts), kw["fanout"], kw["asz"], kw["seed"]))
        return Res(fanouts)

    fanouts = [2, 5, 8, 11, 14]
    out = sw.run_fanout_sweep(None, fanouts, lambda f: dict(fanout=f, asz=12, seed=3), runner=runner)
    assert calls == [(4, [2, 5, 8, 11], 11, 12, 3), (1, [14], 14, 14, 3)]
    assert [int(out.u64(i, "origin")[0]) for i in range(5)] == fanouts


def _replay(yaml_net, tmp_path, plan, gpus=1):
    path, keys, st, pks = yaml_net
    iters, warm, seed = 36, 6, 77
    params = sweep_params(3, 5, iterations=iters, warm_up=warm, step=3, fanout=2)
    sims = oracle_sims(pks, st, params, seed=seed)
    res = str(tmp_path / "r.txt")
    rr.write_results(res, sims)
    args = ["--accounts-from-yaml", "--account-file", path, "--iterations", iters, "--warm-up-rounds", warm,
            "--print-stats", "--replay-results", res, "--seed", seed, "--test-type", "push-fanout",
            "--push-fanout", 2, "--step-size", 3, "--num-simulations", 5, "--origin-rank", 1, 1, 1, 1, 1, 1,
            "--gpus", gpus]
    if plan:
        args += ["--engine-plan", plan]
    return cli(*args)


def test_cli_engine_plan_with_replay(yaml_net, tmp_path):
    """--engine-plan is written before any engine exists, so also from a replayed run."""
    plan = str(tmp_path / "plan.txt")
    with_plan = _replay(yaml_net, tmp_path, plan)
    assert open(plan).read().splitlines() == ["device 0 sims 0,1,2,3 active-set-size 12 fanouts 2,5,8,11",
                                              "device 0 sims 4 active-set-size 14 fanouts 14"]
    without = _replay(yaml_net, tmp_path, None)
    assert with_plan.stdout == without.stdout == ""
    assert rr.report_lines(with_plan.stderr) == rr.report_lines(without.stderr)  # the report is unchanged
    # a group is split into contiguous chunks over --gpus
    _replay(yaml_net, tmp_path, plan, gpus=2)
    assert open(plan).read().splitlines() == ["device 0 sims 0,1 active-set-size 12 fanouts 2,5",
                                              "device 1 sims 2,3 active-set-size 12 fanouts 8,11",
                                              "device 0 sims 4 active-set-size 14 fanouts 14"]


def test_cli_engine_plan_of_the_other_sweeps(yaml_net, tmp_path):
    """One engine per value for active-set-size; one batch for origin-rank."""
    path = yaml_net[0]
    plan = str(tmp_path / "plan.txt")
    res = str(tmp_path / "r.txt")
    rr.write_results(res, [({}, {})] * 3)
    base = ["--accounts-from-yaml", "--account-file", path, "--iterations", 5, "--warm-up-rounds", 5,
            "--replay-results", res, "--engine-plan", plan, "--num-simulations", 3]
    cli(*base, "--test-type", "active-set-size", "--step-size", 2, "--origin-rank", 1, 1, 1, 1)
    assert open(plan).read().splitlines() == [f"device 0 sims {i} active-set-size {12 + 2 * i} fanouts 6"
                                              for i in range(3)]
    cli(*base, "--test-type", "origin-rank", "--origin-rank", 1, 2, 3)
    assert open(plan).read().splitlines() == ["device 0 sims 0,1,2 active-set-size 12 fanouts 6,6,6"]


def test_cli_help_lists_engine_plan():
    assert "--engine-plan" in cli("--help").stdout
