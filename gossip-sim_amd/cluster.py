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
