"""Host arithmetic over the cluster load view (Engine.cluster_load / the cluster_* arrays of
run_simulations(..., cluster=True) / a --cluster-load file): which nodes carry the most when
every node originates, how the load spreads, and how it depends on stake.

Nothing here touches the device; every input is a numpy array indexed by node id."""
import numpy as np

LAMPORTS_PER_SOL = 1_000_000_000
NUM_BUCKETS = 25  # NUM_PUSH_ACTIVE_SET_ENTRIES (push_active_set.rs:11)


def stake_bucket(stake):
    """get_stake_bucket (push_active_set.rs:190-196): bit length of the stake in SOL, at most 24."""
    return min(int(int(stake) // LAMPORTS_PER_SOL).bit_length(), NUM_BUCKETS - 1)


def stake_weights(stakes, origins, scale=1000):
    """Integer weights for a grouped view's slots (Engine.enable_cluster_view(weights=...)) from
    the origins' stakes: max(1, stake * scale // max stake), the largest stake of the WHOLE
    network, in Python integers (no rounding: stake * scale may pass 2^64). So the max-stake node
    weighs `scale`, equal stakes weigh the same and a tiny stake still counts once. u32 [len(origins)]."""
    st = [int(s) for s in np.asarray(stakes, dtype=np.uint64).tolist()]
    scale = int(scale)
    if not st or scale < 1 or scale > 0xFFFFFFFF:
        raise ValueError("stake_weights: needs a network and 1 <= scale < 2^32")
    top = max(st)
    out = []
    for o in origins:
        o = int(o)
        if o < 0 or o >= len(st):
            raise ValueError(f"stake_weights: origin {o} is no node of the network ({len(st)})")
        out.append(max(1, st[o] * scale // top) if top else 1)
    return np.array(out, dtype=np.uint32)


def reach_curve(reach, fractions=(1 / 3, 1 / 2, 2 / 3)):
    """The stake-weighted latency curve of Engine.reach()'s "stake" and "nodes" ([256] per hop
    byte; pass the last_* arrays under these keys for one round's curve). Returns a dict:
      stake / nodes   f64 [255]: the share reached within h hops, h = 0..254, of the total that
                      includes bin 255 (unreached); zeros when the total is 0
      hops_to         {fraction: the smallest h whose cumulative stake is >= fraction x total, or
                      None if no h <= 254 reaches it}, compared in integers (a float fraction is
                      the exact rational it holds)."""
    from fractions import Fraction
    out = {}
    cum = {}
    for k in ("stake", "nodes"):
        a = [int(x) for x in reach[k]]
        if len(a) != 256:
            raise ValueError(f"reach_curve: {k} needs 256 bins")
        total, run, c = sum(a), 0, []
        for x in a[:255]:
            run += x
            c.append(run)
        cum[k] = (c, total)
        out[k] = np.array([float(Fraction(x, total)) if total else 0.0 for x in c])
    c, total = cum["stake"]
    out["hops_to"] = {}
    for f in fractions:
        q = Fraction(f)
        out["hops_to"][f] = next((h for h, x in enumerate(c) if total and x * q.denominator >= q.numerator * total),
                                 None)
    return out


def relay_stake_share(load, total_stake, rounds_weight):
    """Per node, the exact share (fractions.Fraction) of the stake to deliver that heard its
    messages through the node: Engine.tree_stake_load()'s "below" over total_stake x rounds_weight,
    with total_stake the stake one message can reach (the network's, less the origin's where it
    matters) and rounds_weight = recorded rounds x the group's sum of weights (1 with
    "last_below" under the key "below" and unit weights of one slot). Zeros when that product is 0."""
    from fractions import Fraction
    den = int(total_stake) * int(rounds_weight)
    return [Fraction(int(b), den) if den else Fraction(0) for b in load["below"]]


def _spread(a):
    """min / median / p99 / max of a per-node array; the p99 is the value of rank
    ceil(0.99 n) in ascending order (an element of the array, no interpolation)."""
    s = np.sort(np.asarray(a, dtype=np.uint64))
    n = len(s)
    if n == 0:
        return {"min": 0, "median": 0.0, "p99": 0, "max": 0}
    k = max(1, -(-99 * n // 100))
    med = float(s[n // 2]) if n % 2 else (float(s[n // 2 - 1]) + float(s[n // 2])) / 2.0
    return {"min": int(s[0]), "median": med, "p99": int(s[k - 1]), "max": int(s[-1])}


def _top(a, top):
    """[(node, value)] of the `top` largest values, ties by the smaller node id."""
    a = np.asarray(a, dtype=np.uint64)
    order = np.lexsort((np.arange(len(a)), ~a))  # (last key first: ~value ascending = value descending, then id)
    return [(int(v), int(a[v])) for v in order[:max(0, int(top))]]


def summarize(view, stakes, top=10):
    """view: a dict with the u64 [n] arrays egress, ingress, prunes, delivered, hop_sum (more keys
    are ignored), as Engine.cluster_load() returns. Returns a dict:
      top_egress / top_ingress   [(node, total)], the `top` largest, ties by the smaller id
                                 (all n nodes when top > n)
      egress / ingress           {"min", "median", "p99", "max"} over the nodes
      mean_hop                   f64 [n]: hop_sum / delivered, NaN where nothing was delivered
      buckets                    one row per stake bucket that holds a node, ascending:
                                 {"bucket", "nodes", "egress", "ingress", "prunes", "delivered"}
                                 with the mean per node of each total."""
    st = np.asarray(stakes, dtype=np.uint64)
    n = len(st)
    arr = {k: np.asarray(view[k], dtype=np.uint64) for k in ("egress", "ingress", "prunes", "delivered", "hop_sum")}
    for k, a in arr.items():
        if a.shape != (n,):
            raise ValueError(f"summarize: {k} needs one value per node ({n})")
    d = arr["delivered"].astype(np.float64)
    mean_hop = np.full(n, np.nan)
    np.divide(arr["hop_sum"].astype(np.float64), d, out=mean_hop, where=d > 0)
    bk = np.array([stake_bucket(s) for s in st], dtype=np.int64)
    rows = []
    for b in sorted(set(bk.tolist())):
        m = bk == b
        row = {"bucket": int(b), "nodes": int(m.sum())}
        for k in ("egress", "ingress", "prunes", "delivered"):
            row[k] = float(arr[k][m].astype(np.float64).mean())
        rows.append(row)
    return {"top_egress": _top(arr["egress"], top), "top_ingress": _top(arr["ingress"], top),
            "egress": _spread(arr["egress"]), "ingress": _spread(arr["ingress"]), "mean_hop": mean_hop,
            "buckets": rows}
