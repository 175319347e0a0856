"""gossip-sim_amd -- MI355X-native push-propagation engine for gossip-sim.

Python side of the C ABI in include/gossip_hip.h (ctypes, no torch types). The
engine itself is libgossip_hip.so (HIP kernels for gfx950, built in-tree by
`make -C gossip-sim_amd`). There is no CPU fallback: constructing an Engine
without the library or without a visible GPU raises.

The Engine methods mirror the reference's Cluster API (src/gossip.rs):
run_gossip / consume_messages / send_prunes / prune_connections /
chance_to_rotate / fail_nodes, applied to every slot (= independent sim) at once.
"""
import ctypes as C
import os
import subprocess

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG_DIR)
LIB_PATH = os.path.join(PKG_DIR, "libgossip_hip.so")
if os.environ.get("GS_LIB_VARIANT"):  # A/B builds of the same sources (scripts/), never a fallback
    LIB_PATH = os.path.join(PKG_DIR, "variants", os.environ["GS_LIB_VARIANT"], "libgossip_hip.so")

GS_BFS_AUTO, GS_BFS_WORKGROUP, GS_BFS_LEVEL, GS_BFS_BINNED, GS_BFS_MULTI, GS_BFS_HYBRID = 0, 1, 2, 3, 4, 5
GS_FLAG_PROFILE = 1
GS_FLAG_SPLIT_ROUND = 2
GS_FLAG_NARROW_WAVE_PATH = 4
GS_FLAG_BINNED_ALL_LEVELS = 8
GS_FLAG_WIDE_RECORDS = 16
GS_FLAG_NO_SMALL_LEVELS = 32
GS_FLAG_MISPREDICT_LEVELS = 64
GS_FLAG_FRONTIER_EXCHANGE = 128
GS_FLAG_TRAJ_MULTI = 256
HOP_UNREACHED = 0xFF
B58 = "123456789ABCDEFGHJKLMNPQRSTUVWXYZabcdefghijkmnopqrstuvwxyz"


class GsError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"gossip_hip error {code}: {msg}")
        self.code = code


class Params(C.Structure):
    _fields_ = [("push_fanout", C.c_uint32), ("active_set_size", C.c_uint32), ("rotation_probability", C.c_double),
                ("seed", C.c_uint64), ("device", C.c_int32), ("bfs_mode", C.c_uint32),
                ("inbound_capacity", C.c_uint32), ("flags", C.c_uint32)]


class Slot(C.Structure):
    _fields_ = [("origin", C.c_uint32), ("min_ingress_nodes", C.c_uint32), ("prune_stake_threshold", C.c_double)]


class Traj(C.Structure):  # gs_traj: one active-set trajectory table of a gs_create_traj engine
    _fields_ = [("active_set_size", C.c_uint32), ("rotation_probability", C.c_double), ("n_slots", C.c_uint32)]


class RoundSummary(C.Structure):
    _fields_ = [("visited", C.c_uint32), ("pushes", C.c_uint32), ("prunes", C.c_uint32), ("stranded", C.c_uint32),
                ("hop_sum", C.c_uint64), ("hop_count", C.c_uint32), ("hop_min", C.c_uint32),
                ("hop_max", C.c_uint32), ("hop_med_lo", C.c_uint32), ("hop_med_hi", C.c_uint32),
                ("pad0", C.c_uint32), ("stranded_stake_sum", C.c_uint64), ("stranded_stake_min", C.c_uint64),
                ("stranded_stake_max", C.c_uint64), ("stranded_med_lo", C.c_uint64),
                ("stranded_med_hi", C.c_uint64)]


SUMMARY_DTYPE = np.dtype([(n, np.uint32 if t is C.c_uint32 else np.uint64) for n, t in RoundSummary._fields_])
assert SUMMARY_DTYPE.itemsize == C.sizeof(RoundSummary)


class ClusterRound(C.Structure):  # gs_cluster_round: one recorded round of the cluster load view
    _fields_ = [("pushes", C.c_uint64), ("ingress", C.c_uint64), ("prunes", C.c_uint64), ("delivered", C.c_uint64),
                ("egress_max", C.c_uint32), ("egress_max_node", C.c_uint32), ("ingress_max", C.c_uint32),
                ("ingress_max_node", C.c_uint32), ("senders", C.c_uint32), ("pad0", C.c_uint32)]


CLUSTER_ROUND_DTYPE = np.dtype([(n, np.uint32 if t is C.c_uint32 else np.uint64) for n, t in ClusterRound._fields_])
assert CLUSTER_ROUND_DTYPE.itemsize == C.sizeof(ClusterRound)
CLUSTER_TOTALS = ("egress", "ingress", "prunes", "delivered", "hop_sum")
CLUSTER_RESULT_NAMES = tuple("cluster_" + k for k in CLUSTER_TOTALS + (
    "egress_peak", "ingress_peak", "round_pushes", "round_egress_max", "round_egress_max_node", "round_ingress_max",
    "round_ingress_max_node", "round_senders"))


class SimConfig(C.Structure):
    _fields_ = [("push_fanout", C.c_uint32), ("active_set_size", C.c_uint32), ("iterations", C.c_uint32),
                ("warm_up_rounds", C.c_uint32), ("min_ingress_nodes", C.c_uint32), ("when_to_fail", C.c_uint32),
                ("rotation_probability", C.c_double), ("prune_stake_threshold", C.c_double),
                ("fraction_to_fail", C.c_double), ("num_buckets_stranded", C.c_uint64),
                ("num_buckets_message", C.c_uint64), ("num_buckets_hops", C.c_uint64), ("test_type", C.c_int32),
                ("seed", C.c_uint64), ("device", C.c_int32), ("bfs_mode", C.c_uint32)]


EXPORTS = {
    # name: (restype, argtypes)
    "gs_last_error": (C.c_char_p, []),
    "gs_kernel_hash": (C.c_char_p, []),
    "gs_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "gs_read_mst": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p]),
    "gs_create_part": (C.c_int, [C.POINTER(Params), C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                 C.POINTER(C.c_void_p)]),
    "gs_part_sizes": (C.c_int, [C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "gs_part_round": (C.c_int, [C.c_void_p, C.c_uint32, C.c_int, C.POINTER(C.c_uint32)]),
    "gs_part_prunes_out": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "gs_part_prunes_in": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]),
    "gs_part_exchange_sizes": (C.c_int, [C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "gs_part_prunes_dense_out": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "gs_part_prunes_dense_in": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "gs_part_xbfs_groups": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]),
    "gs_part_xbfs_begin": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]),
    "gs_part_xbfs_expand": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p]),
    "gs_part_xbfs_send": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "gs_part_xbfs_apply": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int,
                                     C.POINTER(C.c_uint32)]),
    "gs_part_xbfs_end": (C.c_int, [C.c_void_p, C.c_int]),
    "gs_part_xbfs_expand_async": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p]),
    "gs_part_xbfs_apply_async": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64]),
    "gs_part_xbfs_async_status": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_void_p,
                                            C.c_size_t]),
    "gs_stream": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "gs_part_xround_finish": (C.c_int, [C.c_void_p, C.c_uint32, C.c_int, C.POINTER(C.c_uint32)]),
    "gs_part_stats_out": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "gs_part_stats_in": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "gs_create": (C.c_int, [C.POINTER(Params), C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]),
    "gs_create_traj": (C.c_int, [C.POINTER(Params), C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32,
                                 C.POINTER(C.c_void_p)]),
    "gs_engine_traj": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]),
    "gs_create_traj_seeds": (C.c_int, [C.POINTER(Params), C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32,
                                       C.c_void_p, C.POINTER(C.c_void_p)]),
    "gs_engine_traj_seeds": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]),
    "gs_traj_supported": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_int)]),
    "gs_traj_multi_supported": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
    "gs_set_active_set_entry_traj": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                               C.c_uint32]),
    "gs_get_active_set_entry_traj": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                               C.c_uint32, C.POINTER(C.c_uint32)]),
    "gs_read_active_sets_traj": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "gs_run_simulations_traj": (C.c_int, [C.POINTER(SimConfig), C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.POINTER(C.c_void_p)]),
    "gs_run_simulations_seeds": (C.c_int, [C.POINTER(SimConfig), C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.POINTER(C.c_void_p)]),
    "gs_run_simulations_cluster": (C.c_int, [C.POINTER(SimConfig), C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    "gs_cluster_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "gs_read_cluster_load": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p]),
    "gs_read_cluster_rounds": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "gs_run_simulations_cluster_tables": (C.c_int, [C.POINTER(SimConfig), C.c_void_p, C.c_uint32, C.c_uint32,
                                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                    C.POINTER(C.c_void_p)]),
    "gs_cluster_enable_groups": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "gs_cluster_groups": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.c_void_p]),
    "gs_read_cluster_load_group": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_void_p]),
    "gs_read_cluster_rounds_group": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t,
                                               C.POINTER(C.c_size_t)]),
    "gs_destroy": (None, [C.c_void_p]),
    "gs_set_slots": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32]),
    "gs_set_slot_fanouts": (C.c_int, [C.c_void_p, C.c_void_p]),
    "gs_get_slot_fanouts": (C.c_int, [C.c_void_p, C.c_void_p]),
    "gs_sync": (C.c_int, [C.c_void_p]),
    "gs_init_active_sets": (C.c_int, [C.c_void_p]),
    "gs_set_active_set_entry": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32]),
    "gs_get_active_set_entry": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32,
                                          C.POINTER(C.c_uint32)]),
    "gs_fail_nodes": (C.c_int, [C.c_void_p, C.c_void_p]),
    "gs_run_gossip": (C.c_int, [C.c_void_p]),
    "gs_consume_messages": (C.c_int, [C.c_void_p]),
    "gs_send_prunes": (C.c_int, [C.c_void_p]),
    "gs_prune_connections": (C.c_int, [C.c_void_p]),
    "gs_chance_to_rotate": (C.c_int, [C.c_void_p, C.c_uint32]),
    "gs_record_round": (C.c_int, [C.c_void_p]),
    "gs_round": (C.c_int, [C.c_void_p, C.c_uint32, C.c_int]),
    "gs_read_hops": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p]),
    "gs_read_inbound": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "gs_read_prunes": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_size_t,
                                 C.POINTER(C.c_size_t)]),
    "gs_read_cache": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.c_void_p, C.c_void_p,
                                C.c_uint32, C.POINTER(C.c_uint32)]),
    "gs_read_pruned": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]),
    "gs_read_counters": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gs_read_active_sets": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "gs_read_caches": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gs_read_pruned_all": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p]),
    "gs_read_round_summaries": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "gs_read_accumulators": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p]),
    "gs_read_failed": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p]),
    "gs_kernel_time": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    "gs_kernel_time_reset": (C.c_int, [C.c_void_p]),
    "gs_engine_round_kind": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]),
    "gs_engine_bfs_geometry": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "gs_engine_round_split": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "gs_engine_memory": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "gs_engine_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                 C.POINTER(C.c_uint64)]),
    "gs_hops_stat_new": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p]),
    "gs_stat_collection_calculate": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p]),
    "gs_run_simulations": (C.c_int, [C.POINTER(SimConfig), C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    "gs_run_simulations_fanouts": (C.c_int, [C.POINTER(SimConfig), C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    "gs_result_free": (None, [C.c_void_p]),
    "gs_result_f64": (C.c_size_t, [C.c_void_p, C.c_uint32, C.c_char_p, C.c_void_p, C.c_size_t]),
    "gs_result_u64": (C.c_size_t, [C.c_void_p, C.c_uint32, C.c_char_p, C.c_void_p, C.c_size_t]),
}

_lib = None


def source_hash():
    """sha256 (16 hex digits) of the device sources on disk (csrc/*.hip, csrc/*.h), hashed
    as gen_khash.py hashes them when the library is built."""
    import hashlib
    h = hashlib.sha256()
    d = os.path.join(PKG_DIR, "csrc")
    for name in sorted(os.listdir(d)):
        if name.endswith((".hip", ".h")):
            h.update(name.encode() + b"\0")
            with open(os.path.join(d, name), "rb") as f:
                h.update(f.read())
    return h.hexdigest()[:16]


def kernel_hash():
    """The kernel hash compiled into the LOADED libgossip_hip.so (gs_kernel_hash), when it
    equals the sources on disk; None under GS_LIB_VARIANT (an A/B build) or when the library
    is out of date with its sources. Profiles under profiles/ carry the hash of the kernels
    they measured; bench.py reports a profile's figures only when it equals this one."""
    if os.environ.get("GS_LIB_VARIANT"):
        return None
    built = lib().gs_kernel_hash().decode()
    return built if built == source_hash() else None


def build(quiet=True):
    """Compile libgossip_hip.so (and the gossip-sim CLI) for gfx950 in-tree."""
    cmd = ["make", "-C", PKG_DIR, "-j8"]
    subprocess.check_call(cmd, stdout=subprocess.DEVNULL if quiet else None)


def lib():
    """Load the engine library; raises if it is missing (no fallback path)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise GsError(-2, f"{LIB_PATH} is missing: run `make -C gossip-sim_amd` (no CPU fallback exists)")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in EXPORTS.items():
            f = getattr(L, name, None)
            if f is None and os.environ.get("GS_LIB_VARIANT"):
                continue  # (an A/B build of older sources may predate a symbol; calling it still raises)
            if f is None:
                raise GsError(-2, f"{LIB_PATH} does not export {name}: rebuild it (`make -C gossip-sim_amd`)")
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _check(rc):
    if rc != 0:
        raise GsError(rc, lib().gs_last_error().decode())


def b58encode(b: bytes) -> str:
    n = int.from_bytes(b, "big")
    s = ""
    while n:
        n, r = divmod(n, 58)
        s = B58[r] + s
    return "1" * (len(b) - len(b.lstrip(b"\x00"))) + s


def ids_from_pubkeys(pubkeys):
    """Node id = rank of the base58 string (the consume tie-break order, gossip.rs:639-645)."""
    strs = [b58encode(p) for p in pubkeys]
    order = sorted(range(len(strs)), key=lambda i: strs[i])
    ids = [0] * len(strs)
    for r, i in enumerate(order):
        ids[i] = r
    return ids


def traj_supported(n, fanout, max_asz):
    """(supported, fused): can a network of n nodes run as a trajectory-table engine with this
    push-fanout capacity and largest active-set size, and would its round be the one-kernel
    one. Host arithmetic of the workgroup engine's LDS rule; needs no device."""
    fused = C.c_int()
    ok = lib().gs_traj_supported(int(n), int(fanout), int(max_asz), C.byref(fused))
    return bool(ok), bool(fused.value)


def traj_multi_supported(n, n_slots, fanout, max_asz):
    """Can a network of n nodes run as a multi-source trajectory-table engine (Engine(...,
    trajectories=, traj_multi=True, bfs_mode=GS_BFS_MULTI)) of n_slots slots with this push-fanout
    capacity and largest active-set size. Host arithmetic of the multi-source BFS's geometry
    rule; needs no device."""
    return bool(lib().gs_traj_multi_supported(int(n), int(n_slots), int(fanout), int(max_asz)))


class Engine:
    """One engine = one device + n_slots sims on one shared active-set trajectory, or, with
    trajectories=[(active_set_size, rotation_probability, n_slots), ...], on several tables:
    table t serves the next n_slots slots (their counts sum to the engine's), the capacity is
    the largest size, and `active_set_size` / `rotation_probability` are unused. traj_multi=True
    (GS_FLAG_TRAJ_MULTI) lets the tables live on the multi-source BFS: bfs_mode=GS_BFS_MULTI at
    any size it supports, AUTO beyond the workgroup engine. Tuples of four, (active_set_size,
    rotation_probability, n_slots, seed), give every table its own Philox key (gs_create_traj_seeds;
    `seed` is then unused): a slot of such a table equals an Engine(seed=that seed) at its size and
    probability. If any tuple carries a seed, all must."""

    def __init__(self, stakes, n_slots, *, fanout=6, active_set_size=12, rotation_probability=0.013333, seed=0,
                 device=0, bfs_mode=GS_BFS_AUTO, inbound_capacity=0, profile=False, split_round=False,
                 narrow_wave_path=False, binned_all_levels=False, wide_records=False, no_small_levels=False,
                 mispredict_levels=False, frontier_exchange=False, part=None, trajectories=None, traj_multi=False):
        L = lib()
        if trajectories is not None:
            if part is not None:
                raise ValueError("Engine: partition ranks take no trajectory tables")
            trajectories = [tuple(t) for t in trajectories]
            if len({len(t) for t in trajectories}) > 1 or any(len(t) not in (3, 4) for t in trajectories):
                raise ValueError("Engine: trajectories are (active_set_size, rotation_probability, n_slots) or, for "
                                 "every table, (active_set_size, rotation_probability, n_slots, seed)")
            tseeds = None
            if trajectories and len(trajectories[0]) == 4:
                tseeds = np.array([int(t[3]) for t in trajectories], dtype=np.uint64)
            trajectories = [(int(t[0]), float(t[1]), int(t[2])) for t in trajectories]
            active_set_size = max([a for a, _, _ in trajectories], default=active_set_size)
        self.stakes = np.ascontiguousarray(stakes, dtype=np.uint64)
        self.n = len(self.stakes)
        self.n_slots = n_slots
        self.active_set_size = active_set_size
        p = Params(fanout, active_set_size, rotation_probability, seed, device, bfs_mode, inbound_capacity,
                   (GS_FLAG_PROFILE if profile else 0) | (GS_FLAG_SPLIT_ROUND if split_round else 0) |
                   (GS_FLAG_NARROW_WAVE_PATH if narrow_wave_path else 0) |
                   (GS_FLAG_BINNED_ALL_LEVELS if binned_all_levels else 0) |
                   (GS_FLAG_WIDE_RECORDS if wide_records else 0) | (GS_FLAG_NO_SMALL_LEVELS if no_small_levels else 0) |
                   (GS_FLAG_MISPREDICT_LEVELS if mispredict_levels else 0) |
                   (GS_FLAG_FRONTIER_EXCHANGE if frontier_exchange else 0) |
                   (GS_FLAG_TRAJ_MULTI if traj_multi else 0))
        h = C.c_void_p()
        if trajectories is not None:
            arr = (Traj * max(1, len(trajectories)))(*[Traj(a, q, k) for a, q, k in trajectories])
            if tseeds is not None:
                _check(L.gs_create_traj_seeds(C.byref(p), _ptr(self.stakes), self.n, n_slots, C.cast(arr, C.c_void_p),
                                              len(trajectories), _ptr(tseeds), C.byref(h)))
            else:
                _check(L.gs_create_traj(C.byref(p), _ptr(self.stakes), self.n, n_slots, C.cast(arr, C.c_void_p),
                                        len(trajectories), C.byref(h)))
        elif part is None:
            _check(L.gs_create(C.byref(p), _ptr(self.stakes), self.n, n_slots, C.byref(h)))
        else:  # (rank, nranks): one rank of a node-range partition (gossip_sim_amd.partition)
            _check(L.gs_create_part(C.byref(p), _ptr(self.stakes), self.n, n_slots, part[0], part[1], C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            lib().gs_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def info(self):
        n, s, m, b = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint64()
        _check(lib().gs_engine_info(self.h, C.byref(n), C.byref(s), C.byref(m), C.byref(b)))
        f = C.c_uint32()
        _check(lib().gs_engine_round_kind(self.h, C.byref(f)))
        pb, ob = C.c_uint64(), C.c_uint64()
        _check(lib().gs_engine_memory(self.h, C.byref(pb), C.byref(ob)))
        sp = np.zeros(3, dtype=np.uint32)  # round split (GS_ROUND_SPLIT): on, slots of the two groups
        fn = getattr(lib(), "gs_engine_round_split", None)  # (None: an A/B build of older sources)
        if fn is not None:
            _check(fn(self.h, _ptr(sp), 3))
        return {"n_nodes": n.value, "n_slots": s.value, "bfs_mode": m.value, "device_bytes": b.value,
                "pair_bytes": pb.value, "other_bytes": ob.value, "fused_round": bool(f.value),
                "bfs_persistent": bool(self.bfs_geometry()["persistent_wgs"]),
                "round_split": bool(sp[0]), "round_split_groups": [int(sp[1]), int(sp[2])] if sp[0] else []}

    def bfs_geometry(self):
        """Multi / hybrid BFS geometry (diagnostics): expand slice, coarse and fine bins, group width, groups."""
        out = np.zeros(6, dtype=np.uint32)
        _check(lib().gs_engine_bfs_geometry(self.h, _ptr(out), 6))
        return dict(zip(["expand_slice", "coarse_bins", "fine_bins", "group_width", "groups", "persistent_wgs"],
                        out.tolist()))

    def set_slots(self, origins, min_ingress=2, thresholds=0.15):
        S = self.n_slots
        mi = np.broadcast_to(np.asarray(min_ingress), (S,))
        th = np.broadcast_to(np.asarray(thresholds, dtype=np.float64), (S,))
        arr = (Slot * S)(*[Slot(int(o), int(m), float(t)) for o, m, t in zip(origins, mi, th)])
        _check(lib().gs_set_slots(self.h, C.cast(arr, C.c_void_p), S))

    def set_slot_fanouts(self, fanouts):
        """Per-slot push fanouts, each in [1, the engine's `fanout`] (its capacity); None restores
        the uniform value. Takes effect at the next run_gossip / round."""
        if fanouts is None:
            _check(lib().gs_set_slot_fanouts(self.h, None))
            return
        f = np.ascontiguousarray(fanouts, dtype=np.uint32)
        if f.shape != (self.n_slots,):
            raise ValueError(f"set_slot_fanouts: need exactly {self.n_slots} values")
        _check(lib().gs_set_slot_fanouts(self.h, _ptr(f)))

    def slot_fanouts(self):
        out = np.zeros(self.n_slots, dtype=np.uint32)
        _check(lib().gs_get_slot_fanouts(self.h, _ptr(out)))
        return out

    def init_active_sets(self):
        _check(lib().gs_init_active_sets(self.h))

    def trajectories(self):
        """The engine's tables: [(active_set_size, rotation_probability, n_slots), ...]."""
        n = C.c_uint32()
        arr = (Traj * 256)()
        _check(lib().gs_engine_traj(self.h, C.cast(arr, C.c_void_p), 256, C.byref(n)))
        return [(arr[t].active_set_size, arr[t].rotation_probability, arr[t].n_slots) for t in range(n.value)]

    def table_seeds(self):
        """The Philox key of each table (the engine's seed for every table of an engine made
        without per-table seeds)."""
        n = C.c_uint32()
        out = np.zeros(max(1, self.n_slots), dtype=np.uint64)
        _check(lib().gs_engine_traj_seeds(self.h, _ptr(out), len(out), C.byref(n)))
        return [int(x) for x in out[:n.value]]

    def set_entry(self, node, bucket, peers, table=None):
        a = np.ascontiguousarray(peers, dtype=np.uint32)
        if table is None:
            _check(lib().gs_set_active_set_entry(self.h, node, bucket, _ptr(a), len(a)))
        else:
            _check(lib().gs_set_active_set_entry_traj(self.h, table, node, bucket, _ptr(a), len(a)))

    def get_entry(self, node, bucket, table=None):
        out = np.zeros(64, dtype=np.uint32)
        ln = C.c_uint32()
        if table is None:
            _check(lib().gs_get_active_set_entry(self.h, node, bucket, _ptr(out), 64, C.byref(ln)))
        else:
            _check(lib().gs_get_active_set_entry_traj(self.h, table, node, bucket, _ptr(out), 64, C.byref(ln)))
        return [int(x) for x in out[:ln.value]]

    def fail_nodes(self, fractions):
        f = np.ascontiguousarray(np.broadcast_to(np.asarray(fractions, dtype=np.float64), (self.n_slots,)))
        _check(lib().gs_fail_nodes(self.h, _ptr(f)))

    # --- Cluster steps -------------------------------------------------------
    def run_gossip(self):
        _check(lib().gs_run_gossip(self.h))

    def consume_messages(self):
        _check(lib().gs_consume_messages(self.h))

    def send_prunes(self):
        _check(lib().gs_send_prunes(self.h))

    def prune_connections(self):
        _check(lib().gs_prune_connections(self.h))

    def chance_to_rotate(self, round_index):
        _check(lib().gs_chance_to_rotate(self.h, round_index))

    def record_round(self):
        _check(lib().gs_record_round(self.h))

    def round(self, round_index, record=False):
        _check(lib().gs_round(self.h, round_index, 1 if record else 0))

    def sync(self):
        _check(lib().gs_sync(self.h))

    # --- readbacks -----------------------------------------------------------
    def hops(self, slot):
        out = np.zeros(self.n, dtype=np.uint8)
        _check(lib().gs_read_hops(self.h, slot, _ptr(out)))
        return out

    def distances(self, slot):
        h = self.hops(slot).astype(np.uint64)
        h[h == HOP_UNREACHED] = np.uint64(2**64 - 1)
        return h

    def inbound(self, slot, cap=None):
        cap = cap or 64 * self.n
        off = np.zeros(self.n + 1, dtype=np.uint32)
        src = np.zeros(cap, dtype=np.uint32)
        hop = np.zeros(cap, dtype=np.uint8)
        _check(lib().gs_read_inbound(self.h, slot, _ptr(off), _ptr(src), _ptr(hop), cap))
        return off, src, hop

    def inbound_lists(self, slot):
        off, src, hop = self.inbound(slot)
        return [list(zip(src[off[v]:off[v + 1]].tolist(), hop[off[v]:off[v + 1]].tolist())) for v in range(self.n)]

    def prunes(self, slot):
        cap = 96 * self.n
        a = np.zeros(cap, dtype=np.uint32)
        b = np.zeros(cap, dtype=np.uint32)
        cnt = C.c_size_t()
        _check(lib().gs_read_prunes(self.h, slot, _ptr(a), _ptr(b), cap, C.byref(cnt)))
        return list(zip(a[:cnt.value].tolist(), b[:cnt.value].tolist()))

    def cache(self, slot, node):
        up, ln = C.c_uint32(), C.c_uint32()
        k = np.zeros(128, dtype=np.uint32)
        s = np.zeros(128, dtype=np.uint32)
        _check(lib().gs_read_cache(self.h, slot, node, C.byref(up), _ptr(k), _ptr(s), 128, C.byref(ln)))
        return up.value, dict(zip(k[:ln.value].tolist(), s[:ln.value].tolist()))

    def pruned(self, slot, node):
        m = C.c_uint32()
        _check(lib().gs_read_pruned(self.h, slot, node, C.byref(m)))
        return m.value

    def active_sets(self, table=None):
        """(peers[n, 25, asz] FIFO order, lens[n, 25]); table: one of a trajectory-table engine's
        (asz is then that table's own size)."""
        asz = self.active_set_size
        if table is not None:
            tr = self.trajectories()
            asz = tr[table][0] if 0 <= table < len(tr) else asz  # (out of range: refused by the call below)
        peers = np.zeros(self.n * 25 * asz, dtype=np.uint32)
        lens = np.zeros(self.n * 25, dtype=np.uint8)
        if table is None:
            _check(lib().gs_read_active_sets(self.h, _ptr(peers), _ptr(lens)))
        else:
            _check(lib().gs_read_active_sets_traj(self.h, table, _ptr(peers), _ptr(lens)))
        return peers.reshape(self.n, 25, asz), lens.reshape(self.n, 25)

    def caches(self, slot):
        """(upserts[n], lens[n], keys[n, 96], scores[n, 96]); keys sorted per node."""
        up = np.zeros(self.n, dtype=np.uint32)
        ln = np.zeros(self.n, dtype=np.uint32)
        k = np.zeros(self.n * 96, dtype=np.uint32)
        s = np.zeros(self.n * 96, dtype=np.uint32)
        _check(lib().gs_read_caches(self.h, slot, _ptr(up), _ptr(ln), _ptr(k), _ptr(s)))
        return up, ln, k.reshape(self.n, 96), s.reshape(self.n, 96)

    def pruned_all(self, slot):
        out = np.zeros(self.n, dtype=np.uint32)
        _check(lib().gs_read_pruned_all(self.h, slot, _ptr(out)))
        return out

    def counters(self, slot):
        e = np.zeros(self.n, dtype=np.uint32)
        i = np.zeros(self.n, dtype=np.uint32)
        p = np.zeros(self.n, dtype=np.uint32)
        _check(lib().gs_read_counters(self.h, slot, _ptr(e), _ptr(i), _ptr(p)))
        return e, i, p

    def summaries(self):
        cap = 1 << 16
        while True:
            out = np.zeros(cap, dtype=SUMMARY_DTYPE)
            cnt = C.c_size_t()
            rc = lib().gs_read_round_summaries(self.h, _ptr(out), cap, C.byref(cnt))
            if rc == -4 and cnt.value > cap:
                cap = cnt.value
                continue
            _check(rc)
            return out[:cnt.value].reshape(-1, self.n_slots)

    def mst(self, slot):
        """Cluster::mst (gossip.rs:580-591): {discoverer: sorted nodes it first discovered}."""
        parent = np.zeros(self.n, dtype=np.uint32)
        _check(lib().gs_read_mst(self.h, slot, _ptr(parent)))
        out = {}
        for v in np.nonzero(parent != 0xFFFFFFFF)[0]:
            out.setdefault(int(parent[v]), []).append(int(v))
        return out

    def pushes(self, slot):
        """Cluster::pushes (gossip.rs:566-573): {src: sorted peers it pushed to}."""
        off, src, _ = self.inbound(slot)
        out = {}
        for v in range(self.n):
            for s in src[off[v]:off[v + 1]].tolist():
                out.setdefault(int(s), []).append(v)
        return {k: sorted(v) for k, v in out.items()}

    def accumulators(self, slot):
        e = np.zeros(self.n, dtype=np.uint64)
        i = np.zeros(self.n, dtype=np.uint64)
        p = np.zeros(self.n, dtype=np.uint64)
        st = np.zeros(self.n, dtype=np.uint32)
        hh = np.zeros(256, dtype=np.uint64)
        _check(lib().gs_read_accumulators(self.h, slot, _ptr(e), _ptr(i), _ptr(p), _ptr(st), _ptr(hh)))
        return e, i, p, st, hh

    # --- cluster load view (per-node load summed over every slot) --------------
    def enable_cluster_view(self, on=True, groups=None, weights=None):
        """Allocates (or, on=False, frees) the cluster load view: from now on every recorded round
        also sums the slots' egress / ingress / prunes / deliveries per node on the device.
        groups: slot counts of consecutive slot groups (they sum to n_slots), or "tables" for one
        group per trajectory table; weights: a u32 per slot (0 excludes the slot; default 1). With
        either, every group keeps its own totals, peaks and rounds (cluster_load(group) ...)."""
        if not on:
            if groups is not None or weights is not None:
                raise ValueError("enable_cluster_view: groups / weights go with on=True")
            _check(lib().gs_cluster_enable(self.h, 0))
            return
        if groups is None and weights is None:
            _check(lib().gs_cluster_enable(self.h, 1))
            return
        g, w = cluster_group_args(self.n_slots, groups, weights)
        _check(lib().gs_cluster_enable_groups(self.h, None if g is None else _ptr(g), 0 if g is None else len(g),
                                              None if w is None else _ptr(w)))

    def cluster_groups(self):
        """(slot counts of the enabled view's groups, the slots' weights): both u32 arrays."""
        g = np.zeros(self.n_slots, dtype=np.uint32)  # (at most a group per slot)
        w = np.zeros(self.n_slots, dtype=np.uint32)
        cnt = C.c_uint32()
        _check(lib().gs_cluster_groups(self.h, _ptr(g), len(g), C.byref(cnt), _ptr(w)))
        return g[:cnt.value].copy(), w

    def cluster_load(self, group=None):
        """Totals over the recorded rounds since set_slots -- egress, ingress, prunes, delivered,
        hop_sum (u64 [n]) -- and the per-round peaks egress_peak, ingress_peak (u32 [n]); of slot
        group `group` of a grouped view (None: the only group)."""
        out = {k: np.zeros(self.n, dtype=np.uint64) for k in CLUSTER_TOTALS}
        out["egress_peak"] = np.zeros(self.n, dtype=np.uint32)
        out["ingress_peak"] = np.zeros(self.n, dtype=np.uint32)
        ptrs = [_ptr(out[k]) for k in CLUSTER_TOTALS] + [_ptr(out["egress_peak"]), _ptr(out["ingress_peak"])]
        if group is None:
            _check(lib().gs_read_cluster_load(self.h, *ptrs))
        else:
            _check(lib().gs_read_cluster_load_group(self.h, _group_index(group), *ptrs))
        return out

    def cluster_rounds(self, group=None):
        """One CLUSTER_ROUND_DTYPE record per recorded round (row r of summaries() is the same
        round); of slot group `group` of a grouped view (None: the only group)."""
        cap = 1 << 12
        g = None if group is None else _group_index(group)
        while True:
            out = np.zeros(cap, dtype=CLUSTER_ROUND_DTYPE)
            cnt = C.c_size_t()
            if g is None:
                rc = lib().gs_read_cluster_rounds(self.h, _ptr(out), cap, C.byref(cnt))
            else:
                rc = lib().gs_read_cluster_rounds_group(self.h, g, _ptr(out), cap, C.byref(cnt))
            if rc == -4 and cnt.value > cap:
                cap = cnt.value
                continue
            _check(rc)
            return out[:cnt.value]

    def failed(self, slot):
        out = np.zeros(self.n, dtype=np.uint8)
        _check(lib().gs_read_failed(self.h, slot, _ptr(out)))
        return out

    def kernel_time(self, family):
        ms, n = C.c_double(), C.c_uint64()
        _check(lib().gs_kernel_time(self.h, family.encode(), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def kernel_time_reset(self):
        _check(lib().gs_kernel_time_reset(self.h))


def _group_index(group):
    g = int(group)
    if g < 0 or g != group:
        raise ValueError(f"cluster view: group must be a non-negative integer, not {group!r}")
    return g


def _u32_array(what, x):
    a = np.asarray(x)
    if a.ndim != 1 or a.dtype.kind not in "iu" or (a.size and (int(a.min()) < 0 or int(a.max()) > 0xFFFFFFFF)):
        raise ValueError(f"{what} must be a list of integers within [0, 2^32)")
    return np.ascontiguousarray(a, dtype=np.uint32)


def cluster_group_args(n_slots, groups, weights):
    """Checks enable_cluster_view's groups / weights for an engine of n_slots slots (no device
    needed) and returns them as u32 arrays (groups None for "tables" or when only weights are
    given: one group per trajectory table; weights None for unit weights)."""
    g = w = None
    if groups is not None and not (isinstance(groups, str) and groups == "tables"):
        if isinstance(groups, str):
            raise ValueError(f'cluster view: groups is a list of slot counts or "tables", not {groups!r}')
        g = _u32_array("cluster view: groups", groups)
        if len(g) == 0 or len(g) > n_slots:
            raise ValueError(f"cluster view: {len(g)} groups for {n_slots} slots")
        if (g == 0).any():
            raise ValueError(f"cluster view: group {int(np.argmax(g == 0))} is empty")
        if int(g.astype(np.uint64).sum()) != n_slots:
            raise ValueError(f"cluster view: groups sum to {int(g.astype(np.uint64).sum())}, the engine has "
                             f"{n_slots} slots")
    if weights is not None:
        w = _u32_array("cluster view: weights", weights)
        if w.shape != (n_slots,):
            raise ValueError(f"cluster view: weights needs exactly n_slots = {n_slots} values")
    return g, w


class HopsStatOut(C.Structure):
    _fields_ = [("mean", C.c_double), ("median", C.c_double), ("max", C.c_uint64), ("min", C.c_uint64)]


def hops_stat(values):
    """HopsStat::new (gossip_stats.rs:47-98) over raw distances (u64::MAX = unreached)."""
    a = np.ascontiguousarray(values, dtype=np.uint64)
    out = HopsStatOut()
    _check(lib().gs_hops_stat_new(_ptr(a), len(a), C.byref(out)))
    return out.mean, out.median, out.max, out.min


def stat_collection(values):
    a = np.ascontiguousarray(values, dtype=np.float64)
    out = np.zeros(4, dtype=np.float64)
    _check(lib().gs_stat_collection_calculate(_ptr(a), len(a), _ptr(out)))
    return tuple(float(x) for x in out)


class SimResult:
    def __init__(self, h, n_sims):
        self.h = h
        self.n_sims = n_sims

    def __del__(self):
        if getattr(self, "h", None):
            lib().gs_result_free(self.h)

    def f64(self, sim, name, cap=1 << 16):
        out = np.zeros(cap, dtype=np.float64)
        n = lib().gs_result_f64(self.h, sim, name.encode(), _ptr(out), cap)
        if n == C.c_size_t(-1).value:
            raise KeyError(name)
        return out[:n].copy()

    def u64(self, sim, name, cap=1 << 20):
        out = np.zeros(cap, dtype=np.uint64)
        n = lib().gs_result_u64(self.h, sim, name.encode(), _ptr(out), cap)
        if n == C.c_size_t(-1).value:
            raise KeyError(name)
        return out[:n].copy()


def run_simulations(stakes, *, n_sims=1, origin_ranks=None, min_ingress=None, thresholds=None, fractions=None,
                    fanout=6, asz=12, iterations=1, warm_up=200, p=0.013333, thr=0.15, min_ingress_nodes=2,
                    fraction_to_fail=0.1, when_to_fail=0, nb_stranded=10, nb_message=5, nb_hops=15, test_type=0,
                    seed=0, device=0, bfs_mode=GS_BFS_AUTO, fanouts=None, aszs=None, rot_probs=None, seeds=None,
                    cluster=False, cluster_weights=None):
    """gossip_main.rs run_simulation for n_sims sims as slots of one engine.
    fanouts: a push fanout per sim (the engine's capacity is their maximum; `fanout` is unused then).
    aszs / rot_probs: an active-set size / rotation probability per sim (default `asz` / `p`); sims
    with equal pairs share a trajectory table of one engine, and results stay in sim order.
    seeds: a Philox seed per sim (`seed` is unused then): the tables are the distinct (size,
    probability, seed) triples, so seed replicas run as one engine, each sim equal to its own
    run_simulations(seed=...) call.
    cluster: run the engine with its cluster load view on; the result then also answers
    u64(sim, name) for CLUSTER_RESULT_NAMES (the same arrays under every sim). cluster="tables":
    the view is grouped by trajectory table -- the sims of one (size, probability, seed) -- and the
    names under a sim answer with its own group's arrays; cluster_weights: a u32 weight per sim
    (0 excludes the sim from its group's sums; "tables" only)."""
    st = np.ascontiguousarray(stakes, dtype=np.uint64)
    cfg = SimConfig(fanout, asz, iterations, warm_up, min_ingress_nodes, when_to_fail, p, thr, fraction_to_fail,
                    nb_stranded, nb_message, nb_hops, test_type, seed, device, bfs_mode)

    def arr(x, dt):
        return None if x is None else np.ascontiguousarray(x, dtype=dt)

    r, mi, th, fr = arr(origin_ranks, np.uint32), arr(min_ingress, np.uint32), arr(thresholds, np.float64), \
        arr(fractions, np.float64)
    fo = arr(fanouts, np.uint32)
    if fo is not None and fo.shape != (n_sims,):
        raise ValueError(f"run_simulations: fanouts needs exactly n_sims = {n_sims} values")
    az, rp = arr(aszs, np.uint32), arr(rot_probs, np.float64)
    for name, x in (("aszs", az), ("rot_probs", rp)):
        if x is not None and x.shape != (n_sims,):
            raise ValueError(f"run_simulations: {name} needs exactly n_sims = {n_sims} values")
    sd = arr(seeds, np.uint64)
    if sd is not None and sd.shape != (n_sims,):
        raise ValueError(f"run_simulations: seeds needs exactly n_sims = {n_sims} values")
    if isinstance(cluster, str) and cluster != "tables":
        raise ValueError(f'run_simulations: cluster is True, False or "tables", not {cluster!r}')
    by_table = isinstance(cluster, str)
    if cluster_weights is not None and not by_table:
        raise ValueError('run_simulations: cluster_weights needs cluster="tables"')
    cw = None if cluster_weights is None else cluster_group_args(n_sims, None, cluster_weights)[1]
    h = C.c_void_p()
    if by_table:
        _check(lib().gs_run_simulations_cluster_tables(
            C.byref(cfg), _ptr(st), len(st), n_sims, None if r is None else _ptr(r),
            None if mi is None else _ptr(mi), None if th is None else _ptr(th), None if fr is None else _ptr(fr),
            None if fo is None else _ptr(fo), None if az is None else _ptr(az), None if rp is None else _ptr(rp),
            None if sd is None else _ptr(sd), None if cw is None else _ptr(cw), C.byref(h)))
    elif cluster:
        _check(lib().gs_run_simulations_cluster(C.byref(cfg), _ptr(st), len(st), n_sims,
                                                None if r is None else _ptr(r), None if mi is None else _ptr(mi),
                                                None if th is None else _ptr(th), None if fr is None else _ptr(fr),
                                                None if fo is None else _ptr(fo), None if az is None else _ptr(az),
                                                None if rp is None else _ptr(rp), None if sd is None else _ptr(sd),
                                                1, C.byref(h)))
    elif sd is not None:
        _check(lib().gs_run_simulations_seeds(C.byref(cfg), _ptr(st), len(st), n_sims,
                                              None if r is None else _ptr(r), None if mi is None else _ptr(mi),
                                              None if th is None else _ptr(th), None if fr is None else _ptr(fr),
                                              None if fo is None else _ptr(fo), None if az is None else _ptr(az),
                                              None if rp is None else _ptr(rp), _ptr(sd), C.byref(h)))
    elif az is None and rp is None:
        _check(lib().gs_run_simulations_fanouts(C.byref(cfg), _ptr(st), len(st), n_sims,
                                                None if r is None else _ptr(r), None if mi is None else _ptr(mi),
                                                None if th is None else _ptr(th), None if fr is None else _ptr(fr),
                                                None if fo is None else _ptr(fo), C.byref(h)))
    else:
        _check(lib().gs_run_simulations_traj(C.byref(cfg), _ptr(st), len(st), n_sims,
                                             None if r is None else _ptr(r), None if mi is None else _ptr(mi),
                                             None if th is None else _ptr(th), None if fr is None else _ptr(fr),
                                             None if fo is None else _ptr(fo), None if az is None else _ptr(az),
                                             None if rp is None else _ptr(rp), C.byref(h)))
    return SimResult(h, n_sims)
