"""Sweeps sharded over GPUs: one process per GPU, sims dealt round-robin.

SURVEY.md 8(e): the simulations of a sweep (gossip_main.rs:774-951: origin-rank,
active-set-size, min-ingress, push-fanout, prune-threshold, fail-nodes,
rotation-probability test types) are independent units. Every rank runs its
share of them as slots of ONE engine on its own GPU (run_simulations); the
Philox contract makes a sim's result independent of which rank ran it and of
which other sims shared its engine. There is no data-path collective: after the
sims finish, each rank packs its sims' result arrays (integer histograms,
counters and the f64 statistics, the latter as their IEEE bit patterns) into one
zero-padded int64 buffer and a single all-reduce(SUM) assembles every sim on
every rank. Adding zeros to bit patterns is exact, so the assembled results are
bit-identical to a one-GPU run. With the "nccl" backend (RCCL over xGMI on ROCm)
the buffer lives on the rank's GPU; with "gloo" it stays on the host.

Test types whose parameter changes the engine's trajectory (active-set-size,
rotation-probability) give each value its own engine; `run_sweep` takes the values
and deals them out the same way. The push fanout does not: only run_gossip's
.take(fanout) reads it, so the sims of a push-fanout sweep are slots of one engine
with a fanout per slot (run_simulations(fanouts=...)). The reference raises a sim's
active-set size to its fanout (gossip_main.rs:809-811), which does change the
trajectory: `fanout_groups` splits the sweep into the sims that share a size, and
`run_fanout_sweep` runs each such group as one engine.

`run_traj_sweep` batches the engine-changing sweeps too: an engine may hold several
active-set trajectory tables (gs_create_traj), one per (size, probability) pair, so a
rank's whole share of such a sweep runs as one engine (run_simulations(aszs=, rot_probs=))
when the network fits the workgroup engine (`traj_supported`); otherwise the share runs as
`run_sweep` does, one engine per value -- or, with multi=True, as one multi-source table
engine (bfs_mode GS_BFS_MULTI) at any node count that BFS supports (`traj_multi_supported`).

`run_trial_sweep` repeats a sweep at several seeds: a table also carries its own Philox key
(gs_create_traj_seeds, run_simulations(seeds=)), so a rank's share of (value, seed) units is one
engine under the same rules (`trial_batchable`). `run_traj_sweep` keeps treating differing
seeds as a reason for per-value engines.
"""
import numpy as np

from . import GS_BFS_MULTI, run_simulations, traj_multi_supported, traj_supported

F64_NAMES = ["coverage", "rmr", "branching", "hop_mean", "hop_median", "coverage_stats", "rmr_stats",
             "branching_stats", "aggregate_hops", "ldh", "stranded", "stranded_round_mean",
             "stranded_round_median"]
U64_NAMES = ["origin", "hop_max", "hop_min", "aggregate_hops", "ldh", "stranded", "stranded_times",
             "stranded_round_count", "stranded_round_max", "stranded_round_min", "hops_hist", "stranded_hist",
             "egress_hist", "ingress_hist", "prune_hist", "egress_cpb", "validator_hist", "hist_errors",
             "failed_count"]
NAMES = [("f", n) for n in F64_NAMES] + [("u", n) for n in U64_NAMES]


def shard(n_units, rank, world):
    """Units owned by `rank`: round-robin, so a sweep of k*world units is balanced."""
    return list(range(rank, n_units, world))


def shard_range(n_units, rank, world):
    """Contiguous units [lo, hi) owned by `rank` (origin sharding of one network)."""
    return n_units * rank // world, n_units * (rank + 1) // world


def gather_rows(dist, local, n_units, world, *, row_bytes, group=None):
    """local: [rows, n_local * row_bytes] uint8 of this rank's contiguous units
    (shard_range). Returns [rows, n_units * row_bytes] with every rank's columns,
    assembled by one all-reduce(SUM) of a zero-padded int64 buffer (exact: each byte
    has one owner). On the "nccl" backend (RCCL over xGMI) the buffer lives on the
    rank's current GPU."""
    torch, tdist = dist
    rank = tdist.get_rank(group)
    lo, hi = shard_range(n_units, rank, world)
    rows = local.shape[0]
    full = np.zeros((rows, n_units * row_bytes), dtype=np.uint8)
    full[:, lo * row_bytes:hi * row_bytes] = local
    assert (n_units * row_bytes) % 8 == 0
    t = torch.from_numpy(full.view(np.int64).copy())
    if tdist.get_backend(group) == "nccl":
        t = t.to(f"cuda:{torch.cuda.current_device()}")
    tdist.all_reduce(t, op=tdist.ReduceOp.SUM, group=group)
    return t.cpu().numpy().view(np.uint8).reshape(rows, -1)


def _dist_info(group):
    try:
        import torch.distributed as tdist
    except ImportError:
        return None, 0, 1
    if not tdist.is_available() or not tdist.is_initialized():
        return None, 0, 1
    return tdist, tdist.get_rank(group), tdist.get_world_size(group)


def _as_bits(kind, a):
    a = np.ascontiguousarray(a, dtype=np.float64 if kind == "f" else np.uint64)
    return a.view(np.int64)


def _from_bits(kind, a):
    return np.ascontiguousarray(a, dtype=np.int64).view(np.float64 if kind == "f" else np.uint64).copy()


class SweepResult:
    """Per-sim result arrays by name, the same names as SimResult.f64/u64."""

    def __init__(self, per_sim):
        self.per_sim = per_sim  # list of {(kind, name): ndarray}
        self.n_sims = len(per_sim)

    def f64(self, sim, name):
        return self.per_sim[sim][("f", name)]

    def u64(self, sim, name):
        return self.per_sim[sim][("u", name)]


def allreduce_results(local, n_sims, *, group=None, device=None):
    """local: {sim index: {(kind, name): ndarray}} for this rank's sims. Returns a
    SweepResult holding every sim, assembled with one all-reduce of lengths and
    one all-reduce of the packed int64 bit patterns."""
    tdist, rank, world = _dist_info(group)
    nn = len(NAMES)
    lens = np.zeros((n_sims, nn), dtype=np.int64)
    for i, arrs in local.items():
        for j, key in enumerate(NAMES):
            lens[i, j] = len(arrs[key])
    if tdist is not None:  # (a one-rank group still runs the collective: RCCL is exercised)
        import torch
        t = torch.from_numpy(lens).to(device) if device is not None else torch.from_numpy(lens)
        tdist.all_reduce(t, op=tdist.ReduceOp.SUM, group=group)
        lens = t.cpu().numpy()
    offs = np.zeros(n_sims * nn + 1, dtype=np.int64)
    np.cumsum(lens.reshape(-1), out=offs[1:])
    buf = np.zeros(int(offs[-1]), dtype=np.int64)
    for i, arrs in local.items():
        for j, (kind, name) in enumerate(NAMES):
            k = i * nn + j
            buf[offs[k]:offs[k + 1]] = _as_bits(kind, arrs[(kind, name)])
    if tdist is not None:  # (a one-rank group still runs the collective: RCCL is exercised)
        import torch
        t = torch.from_numpy(buf).to(device) if device is not None else torch.from_numpy(buf)
        tdist.all_reduce(t, op=tdist.ReduceOp.SUM, group=group)
        buf = t.cpu().numpy()
    per_sim = []
    for i in range(n_sims):
        d = {}
        for j, (kind, name) in enumerate(NAMES):
            k = i * nn + j
            d[(kind, name)] = _from_bits(kind, buf[offs[k]:offs[k + 1]])
        per_sim.append(d)
    return SweepResult(per_sim)


def run_sharded(stakes, *, n_sims, origin_ranks=None, min_ingress=None, thresholds=None, fractions=None,
                group=None, device=None, comm_device=None, runner=None, **cfg):
    """run_simulations for n_sims sims dealt over the ranks of `group`.

    device: the HIP device of this rank's engine (default: LOCAL_RANK via cfg or 0).
    comm_device: where the all-reduce buffer lives ("cuda:<i>" for RCCL, None for gloo).
    runner: the per-rank sim runner (default: the HIP engine's run_simulations).
    """
    tdist, rank, world = _dist_info(group)
    runner = runner or run_simulations
    mine = shard(n_sims, rank, world)

    def sub(x):
        return None if x is None else [x[i] for i in mine]

    local = {}
    if mine:
        kw = dict(cfg)
        if device is not None:
            kw["device"] = device
        res = runner(stakes, n_sims=len(mine), origin_ranks=sub(origin_ranks), min_ingress=sub(min_ingress),
                     thresholds=sub(thresholds), fractions=sub(fractions), **kw)
        for j, i in enumerate(mine):
            local[i] = {(kind, name): (res.f64(j, name) if kind == "f" else res.u64(j, name))
                        for kind, name in NAMES}
    return allreduce_results(local, n_sims, group=group, device=comm_device)


def fanout_groups(fanouts, asz):
    """Engine plan of a push-fanout sweep: lists of sim indices, one list per engine. Sim
    i runs with active-set size max(asz, fanouts[i]) (gossip_main.rs:809-811); sims of equal
    size form one group, in sim order (groups in order of their first sim)."""
    groups = {}
    for i, f in enumerate(fanouts):
        groups.setdefault(max(int(asz), int(f)), []).append(i)
    return list(groups.values())


def fanout_units(fanouts, asz, world):
    """The engines of a push-fanout sweep over `world` ranks, as (rank, sim indices) in
    engine order: the groups of fanout_groups, dealt round-robin when there are at least
    as many as ranks; with fewer, the largest unit is halved (contiguous sims, the first
    such unit on ties) until every rank has one or only single sims remain."""
    units = fanout_groups(fanouts, asz)
    while len(units) < world:
        k = max(range(len(units)), key=lambda j: (len(units[j]), -j))
        if len(units[k]) < 2:
            break
        u = units[k]
        units[k:k + 1] = [u[:(len(u) + 1) // 2], u[(len(u) + 1) // 2:]]
    return [(j % world, u) for j, u in enumerate(units)]


def run_fanout_sweep(stakes, fanouts, make_cfg, *, group=None, device=None, comm_device=None, runner=None):
    """A push-fanout sweep (test type 3): every group of fanout_groups as ONE engine with a
    fanout per slot, the engines dealt over the ranks (fanout_units). make_cfg(fanout) ->
    kwargs of run_simulations for that value, as for run_sweep; its `asz` (default 12) is
    the size before the reference's raise, and everything but `fanout` / `asz` must agree
    within a group. Results are bit-identical to run_sweep over the same values."""
    tdist, rank, world = _dist_info(group)
    runner = runner or run_simulations
    cfgs = [dict(make_cfg(f)) for f in fanouts]
    base = {c.get("asz", 12) for c in cfgs}
    if len(base) > 1:
        raise ValueError("run_fanout_sweep: make_cfg must give every value the same asz")
    asz = base.pop() if base else 12
    local = {}
    for r, sims in fanout_units(fanouts, asz, world):
        if r != rank:
            continue
        kw = dict(cfgs[sims[0]])
        per_sim = ("origin_ranks", "min_ingress", "thresholds", "fractions")  # (one value per sim: joined)
        skip = ("fanout", "asz", "n_sims") + per_sim
        for i in sims[1:]:
            if {k: v for k, v in cfgs[i].items() if k not in skip} != {k: v for k, v in kw.items() if k not in skip}:
                raise ValueError("run_fanout_sweep: the sims of a group differ in more than the fanout")
        for k in per_sim:
            if kw.get(k) is not None:
                kw[k] = [x for i in sims for x in cfgs[i][k]]
        kw.pop("n_sims", None)
        fo = [int(fanouts[i]) for i in sims]
        kw["fanout"] = max(fo)
        kw["asz"] = max(asz, fo[0])
        if device is not None:
            kw["device"] = device
        res = runner(stakes, n_sims=len(sims), fanouts=fo, **kw)
        for j, i in enumerate(sims):
            local[i] = {(kind, name): (res.f64(j, name) if kind == "f" else res.u64(j, name))
                        for kind, name in NAMES}
    return allreduce_results(local, len(fanouts), group=group, device=comm_device)


def run_sweep(stakes, values, make_cfg, *, group=None, device=None, comm_device=None, runner=None):
    """Engine-changing test types (active-set-size, rotation-probability; a push-fanout
    sweep batches instead, run_fanout_sweep):
    one single-sim engine per value, values dealt round-robin over the ranks.
    make_cfg(value) -> kwargs of run_simulations for that value."""
    tdist, rank, world = _dist_info(group)
    runner = runner or run_simulations
    local = {}
    for i in shard(len(values), rank, world):
        kw = dict(make_cfg(values[i]))
        if device is not None:
            kw["device"] = device
        res = runner(stakes, n_sims=1, **kw)
        local[i] = {(kind, name): (res.f64(0, name) if kind == "f" else res.u64(0, name)) for kind, name in NAMES}
    return allreduce_results(local, len(values), group=group, device=comm_device)


def traj_tables(aszs, rot_probs):
    """Table plan of one trajectory-table engine: [(asz, p, sim indices)], one table per distinct
    (size, probability) pair in order of first occurrence; equal pairs need not be adjacent."""
    tabs = {}
    for i, key in enumerate(zip([int(a) for a in aszs], [float(q) for q in rot_probs])):
        tabs.setdefault(key, []).append(i)
    return [(a, q, sims) for (a, q), sims in tabs.items()]


def traj_units(n_values, world):
    """The engines of a batched sweep over `world` ranks, as (rank, value indices): the values
    dealt round-robin (shard), each rank's share one engine; ranks without a value get none."""
    return [(r, shard(n_values, r, world)) for r in range(world) if shard(n_values, r, world)]


_PER_SIM = ("origin_ranks", "min_ingress", "thresholds", "fractions")  # (one value per sim: joined)
_PER_TABLE = ("fanout", "asz", "p", "n_sims") + _PER_SIM


def _traj_mergeable(cfgs):
    """The kwargs (one single-sim dict per value) differ only in asz / p / fanout and the per-sim lists."""
    if not cfgs:
        return False
    rest = [{k: v for k, v in c.items() if k not in _PER_TABLE} for c in cfgs]
    if any(r != rest[0] for r in rest[1:]) or any(c.get("n_sims", 1) != 1 for c in cfgs):
        return False
    for k in _PER_SIM:
        if len({c.get(k) is None for c in cfgs}) > 1:
            return False
    return True


def traj_batchable(cfgs, n_nodes):
    """Can these run_simulations kwargs (one single-sim dict per value) run as one engine: they
    may differ only in asz / p / fanout (and the per-sim lists), and the network must fit the
    workgroup engine at their largest fanout and size."""
    if not _traj_mergeable(cfgs):
        return False
    return traj_supported(n_nodes, max(c.get("fanout", 6) for c in cfgs), max(c.get("asz", 12) for c in cfgs))[0]


def traj_batchable_multi(cfgs, n_nodes):
    """traj_batchable for the multi-source table engine (bfs_mode GS_BFS_MULTI): the same rule on
    the kwargs, and the network must pass traj_multi_supported with one slot per value at their
    largest fanout and size -- any node count the multi-source BFS supports."""
    if not _traj_mergeable(cfgs):
        return False
    return traj_multi_supported(n_nodes, len(cfgs), max(c.get("fanout", 6) for c in cfgs),
                                max(c.get("asz", 12) for c in cfgs))


def run_traj_sweep(stakes, values, make_cfg, *, group=None, device=None, comm_device=None, runner=None, multi=False,
                   cluster=None):
    """run_sweep with each rank's share as ONE engine of several trajectory tables: the same
    arguments (values dealt round-robin over the ranks, make_cfg(value) -> kwargs of
    run_simulations) and bit-identical results. A share that cannot batch (traj_batchable)
    runs one engine per value, as run_sweep does -- unless multi=True and it passes
    traj_batchable_multi: then it runs as ONE multi-source table engine (bfs_mode GS_BFS_MULTI).
    cluster: passed to every run_simulations call as its `cluster` (True, or "tables" for the view
    per value of a batched share); the runner sees the results with their cluster_* arrays, the
    reduced result keeps NAMES (allreduce_results does not carry the view)."""
    tdist, rank, world = _dist_info(group)
    runner = runner or run_simulations
    local = {}
    mine = shard(len(values), rank, world)
    cfgs = [dict(make_cfg(values[i])) for i in mine]
    batch = len(mine) > 1 and traj_batchable(cfgs, len(stakes))
    as_multi = multi and len(mine) > 1 and not batch and traj_batchable_multi(cfgs, len(stakes))
    if batch or as_multi:
        kw = {k: v for k, v in cfgs[0].items() if k not in _PER_TABLE}
        if as_multi:
            kw["bfs_mode"] = GS_BFS_MULTI
        for k in _PER_SIM:
            if cfgs[0].get(k) is not None:
                kw[k] = [x for c in cfgs for x in c[k]]
        if device is not None:
            kw["device"] = device
        if cluster:
            kw["cluster"] = cluster
        res = runner(stakes, n_sims=len(mine), fanouts=[int(c.get("fanout", 6)) for c in cfgs],
                     aszs=[int(c.get("asz", 12)) for c in cfgs], rot_probs=[float(c.get("p", 0.013333)) for c in cfgs],
                     **kw)
        for j, i in enumerate(mine):
            local[i] = {(kind, name): (res.f64(j, name) if kind == "f" else res.u64(j, name)) for kind, name in NAMES}
    else:
        for i, kw in zip(mine, cfgs):
            if device is not None:
                kw["device"] = device
            if cluster:
                kw["cluster"] = cluster
            res = runner(stakes, n_sims=1, **kw)
            local[i] = {(kind, name): (res.f64(0, name) if kind == "f" else res.u64(0, name)) for kind, name in NAMES}
    return allreduce_results(local, len(values), group=group, device=comm_device)


def _trial_mergeable(cfgs):
    """_traj_mergeable with `seed` counted as a per-table key: a trajectory table carries its own
    Philox seed (gs_create_traj_seeds), so configurations whose seeds differ still merge."""
    return _traj_mergeable([{k: v for k, v in c.items() if k != "seed"} for c in cfgs])


def trial_batchable(cfgs, n_nodes):
    """traj_batchable for (value, seed) units: the kwargs may differ in seed as well as in
    asz / p / fanout (and the per-sim lists); the network rule is the same (seeds do not enter
    the geometry)."""
    if not _trial_mergeable(cfgs):
        return False
    return traj_supported(n_nodes, max(c.get("fanout", 6) for c in cfgs), max(c.get("asz", 12) for c in cfgs))[0]


def trial_batchable_multi(cfgs, n_nodes):
    """traj_batchable_multi for (value, seed) units: seed is a per-table key."""
    if not _trial_mergeable(cfgs):
        return False
    return traj_multi_supported(n_nodes, len(cfgs), max(c.get("fanout", 6) for c in cfgs),
                                max(c.get("asz", 12) for c in cfgs))


def run_trial_sweep(stakes, values, seeds, make_cfg, *, group=None, device=None, comm_device=None, runner=None,
                    multi=False, cluster=None):
    """A sweep repeated at several seeds (the reference's users repeat a configuration and look
    at the spread; here a repeat is a seed). Units are (value, seed) pairs, value-major: result
    index i_value * len(seeds) + i_seed. make_cfg(value) -> kwargs of run_simulations for that
    value (its `seed`, if any, is replaced by the unit's); values=[None] is plain replicas of
    make_cfg(None). Units are dealt round-robin over the ranks (shard) and each rank's share runs
    as ONE engine with a table per (size, probability, seed) when trial_batchable -- or, with
    multi=True, trial_batchable_multi (bfs_mode GS_BFS_MULTI) -- else one engine per unit.
    Results are bit-identical either way. cluster: as in run_traj_sweep."""
    tdist, rank, world = _dist_info(group)
    runner = runner or run_simulations
    seeds = [int(s) for s in seeds]
    n_units = len(values) * len(seeds)
    local = {}
    mine = shard(n_units, rank, world)
    cfgs = []
    for i in mine:
        c = dict(make_cfg(values[i // len(seeds)]))
        c["seed"] = seeds[i % len(seeds)]
        cfgs.append(c)
    batch = len(mine) > 1 and trial_batchable(cfgs, len(stakes))
    as_multi = multi and len(mine) > 1 and not batch and trial_batchable_multi(cfgs, len(stakes))
    if batch or as_multi:
        kw = {k: v for k, v in cfgs[0].items() if k not in _PER_TABLE and k != "seed"}
        if as_multi:
            kw["bfs_mode"] = GS_BFS_MULTI
        for k in _PER_SIM:
            if cfgs[0].get(k) is not None:
                kw[k] = [x for c in cfgs for x in c[k]]
        if device is not None:
            kw["device"] = device
        if cluster:
            kw["cluster"] = cluster
        res = runner(stakes, n_sims=len(mine), fanouts=[int(c.get("fanout", 6)) for c in cfgs],
                     aszs=[int(c.get("asz", 12)) for c in cfgs], rot_probs=[float(c.get("p", 0.013333)) for c in cfgs],
                     seeds=[c["seed"] for c in cfgs], **kw)
        for j, i in enumerate(mine):
            local[i] = {(kind, name): (res.f64(j, name) if kind == "f" else res.u64(j, name)) for kind, name in NAMES}
    else:
        for i, kw in zip(mine, cfgs):
            if device is not None:
                kw["device"] = device
            if cluster:
                kw["cluster"] = cluster
            res = runner(stakes, n_sims=1, **kw)
            local[i] = {(kind, name): (res.f64(0, name) if kind == "f" else res.u64(0, name)) for kind, name in NAMES}
    return allreduce_results(local, n_units, group=group, device=comm_device)
