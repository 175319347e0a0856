"""The stake reach view's host side: the three symbols are declared and bound, and
cluster.reach_curve does its arithmetic in integers (values above 2^64 included)."""
import os
import re

import engine_bind as eb

gs = eb.gs
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gossip_hip.h")


def test_symbols_declared_and_bound():
    with open(HEADER) as f:
        text = f.read()
    for name in ("gs_reach_enable", "gs_reach_enable_groups", "gs_read_reach"):
        assert re.search(r"^int %s\(gs_engine\* e," % name, text, re.M), name
        assert name in gs.EXPORTS


def test_reach_curve():
    import gossip_sim_amd.cluster as cluster
    big = 2**70
    stake = [0] * 256
    stake[0], stake[1], stake[2], stake[3], stake[255] = big, 2 * big, 3 * big + 1, 3 * big - 1, 3 * big
    nodes = [0] * 256
    nodes[0], nodes[1], nodes[2], nodes[3], nodes[255] = 1, 2, 3, 1, 1
    c = cluster.reach_curve({"stake": stake, "nodes": nodes}, fractions=(1 / 12, 0.25, 0.5, 0.75, 0.76))
    assert c["stake"].shape == c["nodes"].shape == (255,)
    assert c["stake"][0] == 1 / 12 and c["stake"][1] == 0.25 and c["stake"][3] == c["stake"][254] == 0.75
    assert c["nodes"].tolist()[:4] == [0.125, 0.375, 0.75, 0.875]
    # (the float 1 / 12 lies just below the rational, which bin 0 holds exactly)
    assert c["hops_to"] == {1 / 12: 0, 0.25: 1, 0.5: 2, 0.75: 3, 0.76: None}
    # one lamport short of the half at hop 2: a float share of 2^70-sized values could not tell
    stake[2], stake[3] = 3 * big - 1, 3 * big + 1
    assert cluster.reach_curve({"stake": stake, "nodes": nodes}, fractions=(0.5,))["hops_to"] == {0.5: 3}
    empty = cluster.reach_curve({"stake": [0] * 256, "nodes": [0] * 256})
    assert not empty["stake"].any() and set(empty["hops_to"].values()) == {None}
