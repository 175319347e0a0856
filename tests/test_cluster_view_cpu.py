"""Host side of the cluster load view, without a GPU: cluster.summarize against hand-computed
values, and the CLI's --cluster-load file replayed from a results file that holds cluster_*
totals (the --save-results format), compared line for line with a restatement here."""
import math
import os

import numpy as np
import pytest

import engine_bind as eb
import report_ref as rr
import test_cli as tc

import gossip_sim_amd.cluster as cl

SOL = 1_000_000_000


# --- cluster.summarize -------------------------------------------------------------------
def test_stake_bucket_is_get_stake_bucket():
    # push_active_set.rs:190-196: bit length of the stake in SOL, capped at 24
    for stake, b in [(0, 0), (SOL - 1, 0), (SOL, 1), (2 * SOL, 2), (3 * SOL, 2), (4 * SOL, 3), (1023 * SOL, 10),
                     (1024 * SOL, 11), ((1 << 23) * SOL, 24), (2**64 - 1, 24)]:
        assert cl.stake_bucket(stake) == b, stake


def test_summarize_hand_computed():
    stakes = np.array([0, SOL, 3 * SOL, 2 * SOL, 5 * SOL], dtype=np.uint64)  # buckets 0, 1, 2, 2, 3
    view = {
        "egress": np.array([7, 9, 9, 0, 2], dtype=np.uint64),   # a tie for the maximum: node 1 before node 2
        "ingress": np.array([4, 4, 4, 4, 4], dtype=np.uint64),  # all equal: id order
        "prunes": np.array([0, 1, 2, 4, 0], dtype=np.uint64),
        "delivered": np.array([2, 0, 4, 1, 3], dtype=np.uint64),  # node 1 never received anything
        "hop_sum": np.array([5, 0, 6, 3, 3], dtype=np.uint64),
        "egress_peak": np.zeros(5, dtype=np.uint32),  # (more keys are ignored)
    }
    s = cl.summarize(view, stakes, top=3)
    assert s["top_egress"] == [(1, 9), (2, 9), (0, 7)]
    assert s["top_ingress"] == [(0, 4), (1, 4), (2, 4)]
    assert s["egress"] == {"min": 0, "median": 7.0, "p99": 9, "max": 9}
    assert s["ingress"] == {"min": 4, "median": 4.0, "p99": 4, "max": 4}
    mh = s["mean_hop"]
    assert mh[0] == 2.5 and math.isnan(mh[1]) and mh[2] == 1.5 and mh[3] == 3.0 and mh[4] == 1.0
    assert s["buckets"] == [
        {"bucket": 0, "nodes": 1, "egress": 7.0, "ingress": 4.0, "prunes": 0.0, "delivered": 2.0},
        {"bucket": 1, "nodes": 1, "egress": 9.0, "ingress": 4.0, "prunes": 1.0, "delivered": 0.0},
        {"bucket": 2, "nodes": 2, "egress": 4.5, "ingress": 4.0, "prunes": 3.0, "delivered": 2.5},
        {"bucket": 3, "nodes": 1, "egress": 2.0, "ingress": 4.0, "prunes": 0.0, "delivered": 3.0},
    ]
    # top-k longer than N: every node, once
    s = cl.summarize(view, stakes, top=10)
    assert s["top_egress"] == [(1, 9), (2, 9), (0, 7), (4, 2), (3, 0)]
    assert cl.summarize(view, stakes, top=0)["top_egress"] == []
    # an even count: the median is the mean of the middle pair; p99 of 4 values is the largest
    even = {k: v[:4] for k, v in view.items()}
    assert cl.summarize(even, stakes[:4])["egress"] == {"min": 0, "median": 8.0, "p99": 9, "max": 9}
    with pytest.raises(ValueError):
        cl.summarize(view, stakes[:4])


def test_summarize_values_beyond_f64():
    big = np.array([2**63 + 1, 2**63 + 2, 2**63], dtype=np.uint64)  # not separable in f64
    view = {k: big for k in ("egress", "ingress", "prunes", "delivered", "hop_sum")}
    s = cl.summarize(view, np.zeros(3, dtype=np.uint64), top=2)
    assert s["top_egress"] == [(1, 2**63 + 2), (0, 2**63 + 1)]
    assert s["egress"]["max"] == 2**63 + 2 and s["egress"]["min"] == 2**63


# --- the CLI: --cluster-load from a results file -------------------------------------------
@pytest.fixture(scope="module")
def net(tmp_path_factory):
    d = tmp_path_factory.mktemp("cluster_acct")
    path = str(d / "accounts.yaml")
    tc.cli("write-accounts", "--synthetic", 60, "--account-file", path)
    pks, st = eb.synth.network(60)
    return path, [eb.gs.b58encode(p) for p in pks], st, pks


NAMES = ["cluster_egress", "cluster_ingress", "cluster_prunes", "cluster_delivered", "cluster_hop_sum"]


def test_cli_cluster_load_replay(net, tmp_path):
    path, keys, st, pks = net
    n, iters, warm, seed, ranks = len(st), 24, 4, 77, [1, 2, 3, 4]
    params = tc.sweep_params(6, 4, iterations=iters, warm_up=warm, step=1, ranks=ranks)
    sims = tc.oracle_sims(pks, st, params, seed=seed)
    plain = str(tmp_path / "plain.txt")
    rr.write_results(plain, sims)
    # two engines' totals (as --gpus 2 leaves them: under the first simulation of each engine)
    rng = np.random.default_rng(3)
    tot = [{k: rng.integers(0, 2**40, n, dtype=np.uint64) for k in NAMES} for _ in range(2)]
    with_cl = [(f, dict(u)) for f, u in sims]
    with_cl[0][1].update(tot[0])
    with_cl[2][1].update(tot[1])
    res = str(tmp_path / "cluster.txt")
    rr.write_results(res, with_cl)
    base = ["--accounts-from-yaml", "--account-file", path, "--iterations", iters, "--warm-up-rounds", warm,
            "--seed", seed, "--test-type", "origin-rank", "--num-simulations", 4, "--origin-rank", *ranks,
            "--print-stats"]
    out = str(tmp_path / "load.csv")
    r1 = tc.cli(*base, "--replay-results", res, "--cluster-load", out)
    want = [",".join([keys[v], str(int(st[v]))] + [str(int(tot[0][k][v]) + int(tot[1][k][v])) for k in NAMES])
            for v in range(n)]
    assert open(out).read().split("\n") == want + [""]
    # without --cluster-load: no file, and the report is the one of the results without the totals
    before = set(os.listdir(tmp_path))
    r2 = tc.cli(*base, "--replay-results", res)
    r3 = tc.cli(*base, "--replay-results", plain)
    assert set(os.listdir(tmp_path)) == before
    assert rr.report_lines(r2.stderr) == rr.report_lines(r3.stderr) == rr.report_lines(r1.stderr)
    # a results file saved without the view cannot give the file
    r4 = tc.cli(*base, "--replay-results", plain, "--cluster-load", str(tmp_path / "none.csv"), check=False)
    assert r4.returncode == 1 and "cluster_" in r4.stderr and not os.path.exists(tmp_path / "none.csv")


def test_cli_help_names_the_flag():
    assert "--cluster-load PATH" in tc.cli("--help").stdout
