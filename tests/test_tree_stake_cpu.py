"""The delivery tree in stake, host side: the four symbols are declared and bound, and
cluster.relay_stake_share divides in integers (values above 2^64 included)."""
import os
import re
from fractions import Fraction

import engine_bind as eb

gs = eb.gs
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gossip_hip.h")


def test_symbols_declared_and_bound():
    with open(HEADER) as f:
        text = f.read()
    for name in ("gs_tree_stake_enable", "gs_tree_stake_enable_groups", "gs_read_tree_stake",
                 "gs_read_tree_stake_group"):
        assert re.search(r"^int %s\(gs_engine\* e," % name, text, re.M), name
        assert name in gs.EXPORTS


def test_relay_stake_share():
    import gossip_sim_amd.cluster as cluster
    total = 2**63 + 5
    share = cluster.relay_stake_share({"below": [0, total, 3 * total, 2**70 + 1]}, total, 6)
    assert share == [0, Fraction(1, 6), Fraction(1, 2), Fraction(2**70 + 1, 6 * total)]
    assert share[3] != Fraction(2**70, 6 * total)  # (one lamport is not lost)
    assert cluster.relay_stake_share({"below": [7, 0]}, total, 0) == [0, 0]
