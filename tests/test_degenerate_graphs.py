"""The two ends of the input space the synthetic networks never reach.

Deep rounds: hops are u8 and 0xFF means unreached, so a round succeeds iff its farthest
reached node is at distance <= 253 (level 254 must be empty); otherwise the round, or
the next sync / readback, returns GS_ERANGE. Every BFS implementation carries its own
guard for that (degenerate_case.VARIANTS names one engine variant per guard); a chain of
depth D (degenerate_case.chain_case) puts each of them at D = 251, 252, 253 (accepted,
bit for bit against the oracle: distances, counters, prunes, the inbound CSR with its
hop-254 record, caches, prune state, per-round summaries, the hop histogram up to bin
253) and at D = 254, 255, 256, 300 (refused; at 256 and 300 a u8 hop would wrap).

Tiny clusters: Philox-initialised networks with fewer nodes than a wave, than the
active-set size, than the fanout (N - 1 <= size rotation, frontier queues shorter than a
wave, a single fine bin, mostly idle lanes), 26 rounds through the round-20 prune wave in
every BFS mode against the oracle, with test_gpu_parity's run_parity / run_fused_parity.

The partition rank's BFS (gs_part_round) is not driven here: the package's partition
driver needs a torch.distributed group, i.e. worker processes (tests/test_partition.py)."""
import numpy as np
import pytest

import degenerate_case as dc
import engine_bind as eb

gs = eb.gs
U64MAX = dc.U64MAX
GS_ERANGE = -4
SUMMARY_FIELDS = ["visited", "pushes", "prunes", "stranded", "hop_sum", "hop_count", "hop_min", "hop_max", "hop_med_lo",
                  "hop_med_hi"]
LONG_CASE_PRUNES = 501  # the oracle's prunees on the D = 253 chain over 24 rounds (all in round 19)


# ------------------------------------------------------- the chain fixture ----
@pytest.mark.parametrize("D", [251, 252, 253])
def test_chain_fixture_oracle(D):
    """The fixture's claims, on the oracle alone: the farthest node is at distance D (D - 1
    from c[1]), exactly `spare` nodes are unreached, level i holds c[i] alone, c[i] hears
    from c[i-1], c[i+1] and c[i+2] at hops i, i + 2, i + 3, and the orders of c[D-1]
    hold (c[D], D + 1): the hop-254 record at D = 253."""
    case = dc.chain_case(D)
    c, n = case["c"], case["n"]
    assert n == D + 1 + case["spare"] <= 341 and sorted(c) == list(range(n))
    assert len(set(int(x) for x in case["stakes"])) == 1
    for k, q in enumerate(dc.chain_rounds(D, 1)[0]):
        d = q["dist"]
        reached = d != U64MAX
        assert int(d[reached].max()) == D - k
        assert int((~reached).sum()) == case["spare"]
        want = np.full(n, U64MAX)
        want[c[:D + 1]] = np.abs(np.arange(D + 1) - k)
        np.testing.assert_array_equal(d, want)
    s = dc.chain_sim(case)
    s.run_gossip(c[0])
    assert (c[D], D + 1) in s.orders(c[D - 1])
    i = D // 2
    assert s.orders(c[i]) == sorted([(c[i - 1], i), (c[i + 1], i + 2), (c[i + 2], i + 3)], key=lambda x: x[1])
    assert all(s.orders(v) is None for v in c[D + 1:])  # the spare nodes are never pushed to
    off, src, hop = s.orders_all(64 * n)
    assert int(hop.max()) == D + 1


def test_chain_long_case_oracle_prunes():
    """The 24-round case of test_hop_limit_through_the_prune_wave prunes (min-ingress 2,
    threshold 0.15): the 20th upsert of every chain node's cache prunes its third pusher,
    251 + 250 prunees in round 19, and the chain stays 253 deep afterwards."""
    rr = dc.chain_rounds(253, 24, every=True)
    per_round = [sum(len(q["prunes"]) for q in rec) for rec in rr]
    assert per_round == [0] * 19 + [LONG_CASE_PRUNES] + [0] * 4
    assert all(int(rec[0]["dist"][rec[0]["dist"] != U64MAX].max()) == 253 for rec in rr)


# ------------------------------------------------- the hop limit on the GPU ----
def compare_round(name, eng, want, n, r, state=False):
    for k, q in enumerate(want):
        msg = f"{name} slot {k} round {r}"
        np.testing.assert_array_equal(eng.distances(k), q["dist"], err_msg=f"hops {msg}")
        e, i, p = eng.counters(k)
        oe, oi, op = q["counters"]
        np.testing.assert_array_equal(e, np.where(oe == U64MAX, 0, oe), err_msg=f"egress {msg}")
        np.testing.assert_array_equal(i, np.where(oi == U64MAX, 0, oi), err_msg=f"ingress {msg}")
        np.testing.assert_array_equal(p, op, err_msg=f"prune counters {msg}")
        assert eng.prunes(k) == q["prunes"], f"prunes {msg}"
        if dc.has_inbound(name):
            w_off, w_src, w_hop = q["orders"]
            off, src, hop = eng.inbound(k, cap=len(w_src) + 1)
            np.testing.assert_array_equal(off, w_off, err_msg=f"in-degrees {msg}")
            np.testing.assert_array_equal(src[:len(w_src)], w_src, err_msg=f"inbound sources {msg}")
            np.testing.assert_array_equal(hop[:len(w_hop)], w_hop, err_msg=f"inbound hops {msg}")
        if state:
            up, ln, keys, sc = eng.caches(k)
            oup, oln, okeys, osc = q["caches"]
            has = oup != 0xFFFFFFFF
            np.testing.assert_array_equal(up[has], oup[has], err_msg=f"upserts {msg}")
            np.testing.assert_array_equal(up[~has], 0, err_msg=f"upserts {msg}")
            np.testing.assert_array_equal(ln, oln, err_msg=f"cache sizes {msg}")
            np.testing.assert_array_equal(keys, okeys, err_msg=f"cache keys {msg}")
            np.testing.assert_array_equal(sc, osc, err_msg=f"cache scores {msg}")
            np.testing.assert_array_equal(eng.pruned_all(k), q["pruned"], err_msg=f"prune state {msg}")


def compare_recorded(name, eng, rr, n):
    """Every recorded round's summary, recomputed from the oracle's distances, and the
    hop-histogram accumulator against a bincount of them."""
    summ = eng.summaries()
    assert summ.shape == (len(rr), 2)
    for r, rec in enumerate(rr):
        for k, q in enumerate(rec):
            want = dc.summary_of(q, n)
            got = {f: int(summ[r, k][f]) for f in SUMMARY_FIELDS}
            assert got == want, f"{name} summary slot {k} round {r}"
    for k in range(2):
        hist = np.zeros(256, dtype=np.uint64)
        for rec in rr:
            d = rec[k]["dist"]
            hist += np.bincount(d[d != U64MAX].astype(np.int64), minlength=256).astype(np.uint64)
        np.testing.assert_array_equal(eng.accumulators(k)[4], hist, err_msg=f"{name} hop histogram slot {k}")


@pytest.mark.gpu
@pytest.mark.parametrize("D", [251, 252, 253])
@pytest.mark.parametrize("name", list(dc.VARIANTS))
def test_hop_limit_accepted(name, D, monkeypatch):
    """Farthest node at distance D <= 253 (D - 1 in the second slot; 252 and 253 sit on
    different phases of the level BFS's four-level poll): three recorded rounds equal the
    oracle's in every BFS implementation."""
    case = dc.chain_case(D)
    rr = dc.chain_rounds(D, 3)
    eng = dc.variant_engine(name, case, monkeypatch)
    try:
        eng.set_slots(case["c"][:2], 2, 0.15)
        for r, rec in enumerate(rr):
            dc.variant_round(name, eng, r)
            compare_round(name, eng, rec, case["n"], r, state=r == len(rr) - 1)
        compare_recorded(name, eng, rr, case["n"])
        if D == 253 and dc.has_inbound(name):
            off, src, hop = eng.inbound(0)
            assert int(hop[:off[-1]].max()) == 254  # c[253] -> c[252]
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("D", [254, 255, 256, 300])
@pytest.mark.parametrize("name", list(dc.VARIANTS))
def test_hop_limit_refused(name, D, monkeypatch):
    """A node at distance D >= 254 (at 254 only in the first slot; at 256 and 300 a u8 hop
    would wrap to 0 or a small value): the round, or at the latest the following sync or
    first readback, fails with GS_ERANGE -- never success with wrong hops."""
    case = dc.chain_case(D)
    eng = dc.variant_engine(name, case, monkeypatch)
    try:
        eng.set_slots(case["c"][:2], 2, 0.15)
        with pytest.raises(gs.GsError) as ei:
            if dc.VARIANTS[name].get("steps"):
                eng.run_gossip()
            else:
                eng.round(0, record=True)
            eng.sync()
            eng.hops(0)
        assert ei.value.code == GS_ERANGE and "253 hops" in str(ei.value), str(ei.value)
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["wg-fused", "level", "multi"])
def test_hop_limit_through_the_prune_wave(name, monkeypatch):
    """D = 253 for 24 rounds, min-ingress 2 and threshold 0.15: the records at hops 253 and
    254 pass through the 20th-upsert prune (test_chain_long_case_oracle_prunes pins the
    oracle's 501 prunees in round 19). Prunes, caches and prune state every round."""
    case = dc.chain_case(253)
    rr = dc.chain_rounds(253, 24, every=True)
    assert sum(len(q["prunes"]) for rec in rr for q in rec) == LONG_CASE_PRUNES > 0
    eng = dc.variant_engine(name, case, monkeypatch)
    try:
        eng.set_slots(case["c"][:2], 2, 0.15)
        for r, rec in enumerate(rr):
            dc.variant_round(name, eng, r)
            compare_round(name, eng, rec, case["n"], r, state=True)
        compare_recorded(name, eng, rr, case["n"])
    finally:
        eng.close()


# ------------------------------------------------------------ tiny clusters ----
# (n, push fanout, active-set size): fanout and size both above the peer count; N - 1 <=
# size in one short wave; N - 1 == size; capacity-32 rows with N - 1 == size; one node
# past a wave
TINY = [(3, 6, 12), (7, 6, 12), (13, 6, 12), (33, 32, 32), (65, 6, 12)]
TINY_MODES = [gs.GS_BFS_WORKGROUP, gs.GS_BFS_LEVEL, gs.GS_BFS_BINNED, gs.GS_BFS_MULTI, gs.GS_BFS_HYBRID]


def tiny_ranks(n):
    return sorted({1, (n + 1) // 2, n})  # the largest and the smallest stake, and a middle rank


@pytest.mark.gpu
@pytest.mark.parametrize("n,fanout,asz", TINY)
@pytest.mark.parametrize("mode", TINY_MODES)
def test_tiny_cluster_round_by_round_parity(mode, n, fanout, asz):
    """26 rounds at rotation probability 0.1 on n Philox-initialised nodes, every step
    against the oracle. The oracle alone (min-ingress 2, threshold 0.15) emits prunes at
    n = 7, 13, 33 and 65 (72, 162, 2,880 and 1,194 over these origins) and none at n = 3:
    three nodes cannot hold two ingress nodes plus a prunee."""
    from test_gpu_parity import run_parity
    total = run_parity(n, tiny_ranks(n), 26, p=0.1, mode=mode, asz=asz, fanout=fanout, full_every=5)
    assert (total > 0) == (n > 3), total


@pytest.mark.gpu
@pytest.mark.parametrize("n,fanout,asz", TINY)
def test_tiny_cluster_fused_round_parity(n, fanout, asz):
    """The same sizes through the one-kernel workgroup round, S = n slots, every node an
    origin (CSR staging with most lanes idle); the first, a middle and the last slot are
    compared. The oracle emits prunes at n = 7, 13, 33 and 65, none at n = 3."""
    from test_gpu_parity import run_fused_parity
    eng, total, _ = run_fused_parity(n, n, 26, fanout=fanout, asz=asz, p=0.1, origins=list(range(n)),
                                     check=tuple(sorted({0, n // 2, n - 1})), full_every=5)
    eng.close()
    assert (total > 0) == (n > 3), total
