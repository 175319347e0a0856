"""bench.py's command line: a plain run times the headline and nothing else, --steps sets the
number of timed steps, and --dump-outputs writes the last timed step's outputs as float
arrays that are identical from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
import engine_bind as eb

gs = eb.gs
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SECONDARY = ("steady_state", "weak_trial", "cpu_baseline_1core", "c4", "c3", "c5")


class FakeEngine:
    """The readbacks dump_outputs uses, with values that name their slot."""
    n, n_slots = 50, 40

    def hops(self, k):
        return np.full(self.n, k, dtype=np.uint8)

    def counters(self, k):
        return tuple(np.full(self.n, 100 * j + k, dtype=np.uint32) for j in range(3))


def test_dump_outputs_all_slots_and_seeded_sample(tmp_path, monkeypatch):
    eng = FakeEngine()
    summ = np.zeros((3, eng.n_slots), dtype=gs.SUMMARY_DTYPE)
    summ["pushes"][-1] = np.arange(eng.n_slots)
    summ["stranded_stake_max"][-1] = 2**63
    monkeypatch.setattr(bench, "DUMP_COUNTER_BYTES", 12 * eng.n * 7)  # room for 7 of the 40 slots
    for d in ("a", "b"):
        bench.dump_outputs(eng, summ, str(tmp_path / d))
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in sorted(os.listdir(tmp_path / "a"))}
    assert sorted(got) == ["counter_slots", "egress", "hop_slots", "hops", "ingress", "prune_counts",
                           "round_summaries"]
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    fields = [f for f in gs.SUMMARY_DTYPE.names if f != "pad0"]
    assert got["round_summaries"].shape == (eng.n_slots, len(fields))
    np.testing.assert_array_equal(got["round_summaries"][:, fields.index("pushes")], np.arange(eng.n_slots))
    assert got["round_summaries"][0, fields.index("stranded_stake_max")] == 2.0**63
    np.testing.assert_array_equal(got["hop_slots"], np.arange(eng.n_slots))  # every slot fits
    np.testing.assert_array_equal(got["hops"][:, 0], np.arange(eng.n_slots))
    cs = got["counter_slots"]
    assert cs.shape == (7,) and np.all(np.diff(cs) > 0) and cs.max() < eng.n_slots
    for j, name in enumerate(("egress", "ingress", "prune_counts")):
        assert got[name].shape == (7, eng.n)
        np.testing.assert_array_equal(got[name][:, 0], 100 * j + cs)
    for name, a in got.items():  # the sample is fixed: a second dump is the same
        np.testing.assert_array_equal(a, np.load(tmp_path / "b" / (name + ".npy")))


def run_bench(*args):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *map(str, args)],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_plain_run_is_headline_only_and_dumps_repeat(tmp_path):
    lines = [run_bench("--nodes", 300, "--steps", 3, "--warmup", 2, "--dump-outputs", tmp_path / d)
             for d in ("a", "b")]
    for d in lines:
        assert d["steps"] == 3 and d["warmup"] == 2 and d["config"]["rounds"] == [2, 5]
        assert d["ms_per_step"] > 0 and d["value"] > 0 and d["unit"] == "edges/s" and d["dtype"] == "u32"
        assert d["higher_is_better"] is True and d["cpu_baseline"] is None
        assert not [k for k in SECONDARY if k in d]
    total = 0
    for f in sorted(os.listdir(tmp_path / "a")):
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype in (np.float32, np.float64)
        np.testing.assert_array_equal(a, b, err_msg=f)
        total += a.nbytes
    assert 0 < total <= 64 << 20
    s = np.load(tmp_path / "a" / "round_summaries.npy")
    h = np.load(tmp_path / "a" / "hops.npy")
    assert s.shape[0] == 300 and h.shape == (300, 300)
    # the summaries and the hop rows describe the same step: visited = nodes with a hop count
    np.testing.assert_array_equal(s[:, 0], (h != gs.HOP_UNREACHED).sum(axis=1))
