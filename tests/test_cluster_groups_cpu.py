"""Host side of the grouped, weighted cluster load view, without a GPU: the chunk plan of
gs_cluster_plan.h (tests/cluster_plan_check.cpp, plain and under the host sanitizers),
cluster.stake_weights against hand-computed values, the argument checks of the Python mirror that
need no device, and the CLI's --cluster-load-by-config file replayed from hand-written results."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import engine_bind as eb
import report_ref as rr
import test_cli as tc

import gossip_sim_amd.cluster as cl

gs = eb.gs
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# --- the chunk plan ------------------------------------------------------------------------
@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_chunk_plan(tmp_path, sanitize):
    """tests/cluster_plan_check.cpp: for (NP, group sizes) cases -- G = 1, G = S, (3,1,3),
    (1,64,5), one group of 3,000, 16 tables of 1, NP from 1 to 10^7 -- every chunk lies in one
    group, the chunks of a group tile it exactly once, none is empty, and the count is within
    want + G. A stand-alone program with its own main; the second build has
    -fsanitize=address,undefined on the host compiler and is run directly."""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "cluster_plan_check")
    # (the sanitizer runtimes linked statically: the program needs nothing loaded before it)
    san = ["-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", *(san if sanitize else []), "-I",
                    os.path.join(ROOT, "gossip-sim_amd", "csrc"), os.path.join(ROOT, "tests", "cluster_plan_check.cpp"),
                    "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr


# --- cluster.stake_weights -------------------------------------------------------------------
def test_stake_weights_hand_computed():
    #          0     1    2    3  4  5      6
    stakes = [1000, 500, 500, 1, 0, 999, 333]
    w = cl.stake_weights(stakes, [0, 1, 2, 3, 4, 5, 6])
    assert w.dtype == np.uint32
    # the max-stake node weighs `scale`; ties are equal; 1 * 1000 // 1000 = 1; 0 -> max(1, 0) = 1
    assert w.tolist() == [1000, 500, 500, 1, 1, 999, 333]
    assert cl.stake_weights(stakes, [6, 0, 6], scale=10).tolist() == [3, 10, 3]  # 3330 // 1000; repeats allowed
    assert cl.stake_weights(stakes, [5, 3], scale=1).tolist() == [1, 1]  # 999 // 1000 = 0 -> 1
    # the maximum is the network's, not the origins'
    assert cl.stake_weights(stakes, [1, 6], scale=100).tolist() == [50, 33]
    assert cl.stake_weights(stakes, []).tolist() == []
    # pure integer arithmetic: stake * scale passes 2^64, and f64 would round 2^64 - 2 up to the maximum
    big = [2**64 - 1, 2**64 - 2, 2**63]
    assert cl.stake_weights(big, [0, 1, 2], scale=2**32 - 1).tolist() == [2**32 - 1, 2**32 - 2, 2**31 - 1]
    assert cl.stake_weights([0, 0], [0, 1]).tolist() == [1, 1]  # an unstaked network
    for bad in (dict(stakes=stakes, origins=[7]), dict(stakes=stakes, origins=[-1]), dict(stakes=[], origins=[]),
                dict(stakes=stakes, origins=[0], scale=0), dict(stakes=stakes, origins=[0], scale=2**32)):
        with pytest.raises(ValueError):
            cl.stake_weights(**bad)


# --- argument checks that need no device --------------------------------------------------------
def test_group_arguments():
    g, w = gs.cluster_group_args(7, [3, 1, 3], [1, 2, 0, 5, 1, 1, 3])
    assert g.dtype == w.dtype == np.uint32 and g.tolist() == [3, 1, 3] and w.tolist() == [1, 2, 0, 5, 1, 1, 3]
    assert gs.cluster_group_args(7, "tables", None) == (None, None)
    g, w = gs.cluster_group_args(7, None, [2**32 - 1] * 7)  # weights alone: the tables' groups
    assert g is None and w.tolist() == [2**32 - 1] * 7
    g, w = gs.cluster_group_args(2, np.array([1, 1], dtype=np.int64), None)
    assert g.tolist() == [1, 1] and w is None
    bad = [
        (7, [3, 1, 2], None),           # sums to 6
        (7, [3, 1, 4], None),           # sums to 8
        (7, [3, 0, 4], None),           # an empty group
        (7, [], None),                  # no group
        (3, [1, 1, 1, 1], None),        # more groups than slots
        (7, [3.5, 3.5], None),          # not integers
        (7, [-1, 8], None),             # negative
        (7, [[7]], None),               # not a list of counts
        (7, "table", None),             # the only word is "tables"
        (7, [7], [1] * 6),              # a weight per slot
        (7, [7], [1] * 8),
        (7, [7], [1, 1, 1, 1, 1, 1, -1]),
        (7, [7], [1, 1, 1, 1, 1, 1, 2**32]),
        (7, [7], [1.0] * 7),
    ]
    for n_slots, groups, weights in bad:
        with pytest.raises(ValueError):
            gs.cluster_group_args(n_slots, groups, weights)
    st = np.ones(4, dtype=np.uint64)
    for kw in (dict(cluster="table"), dict(cluster=True, cluster_weights=[1, 1]), dict(cluster_weights=[1, 1]),
               dict(cluster="tables", cluster_weights=[1]), dict(cluster="tables", cluster_weights=[1, -2])):
        with pytest.raises(ValueError):  # (refused before the library is touched)
            gs.run_simulations(st, n_sims=2, **kw)


# --- the CLI: --cluster-load-by-config from a results file ---------------------------------------
@pytest.fixture(scope="module")
def net(tmp_path_factory):
    d = tmp_path_factory.mktemp("cluster_groups_acct")
    path = str(d / "accounts.yaml")
    tc.cli("write-accounts", "--synthetic", 60, "--account-file", path)
    pks, st = eb.synth.network(60)
    return path, [gs.b58encode(p) for p in pks], st


NAMES = ["cluster_egress", "cluster_ingress", "cluster_prunes", "cluster_delivered", "cluster_hop_sum"]


def test_cli_cluster_load_by_config_replay(net, tmp_path):
    path, keys, st = net
    n = len(st)
    rng = np.random.default_rng(5)
    tot = [{k: rng.integers(0, 2**40, n, dtype=np.uint64) for k in NAMES} for _ in range(3)]
    base = ["--accounts-from-yaml", "--account-file", path, "--iterations", 5, "--warm-up-rounds", 5,
            "--num-simulations", 3, "--origin-rank", 1, 1, 1, 1, "--test-type", "active-set-size", "--step-size", 2]

    def lines(engine, table, t):
        return [",".join([str(engine), str(table), keys[v], str(int(st[v]))] + [str(int(t[k][v])) for k in NAMES])
                for v in range(n)]

    def results(tables):  # three sims; tables: {sim: (table index in its engine, totals)}
        sims = [({}, {}) for _ in range(3)]
        for s, (t, arrs) in tables.items():
            sims[s][1].update(arrs)
            sims[s][1]["cluster_table"] = np.array([t], dtype=np.uint64)
        res = str(tmp_path / f"res{len(os.listdir(tmp_path))}.txt")
        rr.write_results(res, sims)
        return res

    out = str(tmp_path / "by_config.csv")
    # --batch-sweeps --gpus 2: engine 0 holds sim 0, engine 1 sims 1 and 2 as tables 0 and 1
    res = results({0: (0, tot[0]), 1: (0, tot[1]), 2: (1, tot[2])})
    tc.cli(*base, "--batch-sweeps", "--gpus", 2, "--replay-results", res, "--cluster-load-by-config", out)
    assert open(out).read().split("\n") == lines(0, 0, tot[0]) + lines(1, 0, tot[1]) + lines(1, 1, tot[2]) + [""]
    # --batch-sweeps on one device: one engine of three tables
    res = results({0: (0, tot[0]), 1: (1, tot[1]), 2: (2, tot[2])})
    tc.cli(*base, "--batch-sweeps", "--replay-results", res, "--cluster-load-by-config", out)
    assert open(out).read().split("\n") == lines(0, 0, tot[0]) + lines(0, 1, tot[1]) + lines(0, 2, tot[2]) + [""]
    # ... and --cluster-load beside it is the sum over the tables (unit weights: the groups add up)
    both = str(tmp_path / "load.csv")
    tc.cli(*base, "--batch-sweeps", "--replay-results", res, "--cluster-load-by-config", out, "--cluster-load", both)
    assert open(both).read().split("\n") == [
        ",".join([keys[v], str(int(st[v]))] + [str(sum(int(t[k][v]) for t in tot)) for k in NAMES])
        for v in range(n)] + [""]
    # without --batch-sweeps: an engine per value, each with one table
    res = results({0: (0, tot[0]), 1: (0, tot[1]), 2: (0, tot[2])})
    tc.cli(*base, "--replay-results", res, "--cluster-load-by-config", out)
    assert open(out).read().split("\n") == lines(0, 0, tot[0]) + lines(1, 0, tot[1]) + lines(2, 0, tot[2]) + [""]
    # a results file saved with --cluster-load only (totals, no table index) cannot give the file
    sims = [({}, {}) for _ in range(3)]
    sims[0][1].update(tot[0])
    plain = str(tmp_path / "plain.txt")
    rr.write_results(plain, sims)
    none = str(tmp_path / "none.csv")
    r = tc.cli(*base, "--replay-results", plain, "--cluster-load-by-config", none, check=False)
    assert r.returncode == 1 and "cluster_table" in r.stderr and not os.path.exists(none)
    # a table whose totals do not fit the network is refused
    short = {k: v[:-1] for k, v in tot[0].items()}
    res = results({0: (0, short), 1: (0, tot[1]), 2: (0, tot[2])})
    r = tc.cli(*base, "--replay-results", res, "--cluster-load-by-config", none, check=False)
    assert r.returncode == 1 and "cluster_egress" in r.stderr and not os.path.exists(none)


def test_cli_help_names_the_flag():
    h = tc.cli("--help").stdout
    assert "--cluster-load-by-config PATH" in h and "--cluster-load PATH" in h
