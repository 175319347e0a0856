/*
 * gossip_hip.h -- C ABI of the MI355X push-propagation engine for gossip-sim.
 *
 * Drop-in boundary for the per-iteration hot path of gregcusack/gossip-sim
 * (src/gossip_main.rs:449-514). The reference has no FFI seam of its own; every
 * entry point below names the reference method it replaces. A Rust maintainer
 * binds these with `extern "C"` declarations; the C++
 * `gossip-sim` driver and the pytest/ctypes parity tests call them directly.
 *
 * Conventions
 *  - Every int-returning call returns GS_OK (0) or a negative gs_status; the
 *    message of the last failure on this thread is gs_last_error(). Nothing
 *    throws across the ABI.
 *  - Nodes are addressed by id = rank of the node's base58 pubkey string
 *    (so the reference's consume tie-break, gossip.rs:639-645, is id order).
 *    stakes[] is indexed by id.
 *  - One engine = one HIP device + one stream + one shared active-set
 *    trajectory, carrying n_slots independent simulations ("slots"). A slot is
 *    one reference Cluster run: its own origin, prune/cache overlay, failed set
 *    and statistics. Sims that share seed/fanout/active-set-size/rotation
 *    probability (an origin-rank, min-ingress, prune-threshold or fail-nodes
 *    sweep, or "all origins") batch into one engine. The push fanout may also differ per
 *    slot (gs_set_slot_fanouts): it is read only by run_gossip's .take(fanout)
 *    (gossip.rs:527-536), never by initialize_gossip, rotation or the weighted shuffle, so
 *    sims that differ only in fanout share the trajectory too, and a push-fanout sweep
 *    batches like the others (its sims with the same active-set size, see sweep.py).
 *    An engine made by gs_create_traj holds several trajectories (tables), each with its
 *    own active-set size and rotation probability and its own range of slots, so the
 *    sims of an active-set-size or rotate-probability sweep batch as well: on the
 *    workgroup engine, and with GS_FLAG_TRAJ_MULTI on the multi-source BFS at any node
 *    count that BFS supports (gs_traj_multi_supported).
 *  - The engine owns all device memory. Inputs are copied at call time; outputs
 *    go to caller buffers with explicit capacities (too small => GS_ERANGE).
 *  - An engine is not re-entrant; use one engine per device per host thread.
 *  - Randomness follows the Philox determinism contract: results
 *    are a pure function of (stakes, params, slots, call sequence).
 */
#ifndef GOSSIP_HIP_H
#define GOSSIP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum gs_status {
  GS_OK = 0,
  GS_EINVAL = -1,  /* bad argument */
  GS_EHIP = -2,    /* HIP runtime failure (no device, launch error, ...) */
  GS_ENOMEM = -3,  /* device or host allocation failed */
  GS_ERANGE = -4,  /* a capacity or limit was exceeded (see gs_last_error) */
  GS_ESTATE = -5   /* call out of order */
} gs_status;

enum { GS_NUM_BUCKETS = 25, GS_MAX_ACTIVE_SET_SIZE = 32, GS_MAX_NODES = (1 << 24) - 1, GS_HOP_UNREACHED = 0xFF };
/* The hop limit. Hops are u8 and GS_HOP_UNREACHED marks an unreached node: a round
 * succeeds if and only if its farthest reached node is at distance <= 253 in every slot
 * (BFS level 254 is empty; the largest hop an inbound record carries is then 254).
 * Otherwise the round -- or, where the BFS reports through the deferred error word (the
 * one-kernel round, the workgroup BFS, the persistent and predicted level loops), the next
 * gs_sync or readback -- returns GS_ERANGE, in every BFS mode; the engine's results after
 * that error are unspecified (tests/test_degenerate_graphs.py). */
/* BFS strategies (results are identical): WORKGROUP = one workgroup per slot with
 * LDS state (small clusters, many slots); LEVEL = level-synchronous over all
 * slots with a global atomic per push; BINNED = level-synchronous,
 * propagation-blocked (pushes binned by destination range, LDS counters per
 * bin); MULTI = batched multi-source frontier BFS (a frontier entry is a node and
 * the mask of slots reaching it at that level: one row expansion and one record
 * per pushed-to peer serve every such slot; large clusters). AUTO picks
 * WORKGROUP (n <= 8,192 and >= 64 slots), else MULTI (when its bin geometry fits LDS
 * and its level area stays below 2^32 records), else BINNED, else LEVEL.
 * HYBRID = direction-optimizing multi-source BFS over the round's push graph: every node's
 * pushes for every slot built once per round as in-records grouped by destination, then
 * levels carrying only slot masks and distances -- top-down (frontier entries, atomicOr on
 * visited masks) for small frontiers, bottom-up (nodes still missing slots scan their
 * in-records for pushers at the current distance) for large ones -- and one gather. */
enum { GS_BFS_AUTO = 0, GS_BFS_WORKGROUP = 1, GS_BFS_LEVEL = 2, GS_BFS_BINNED = 3, GS_BFS_MULTI = 4,
       GS_BFS_HYBRID = 5 };
enum { GS_FLAG_PROFILE = 1, GS_FLAG_SPLIT_ROUND = 2, GS_FLAG_NARROW_WAVE_PATH = 4, GS_FLAG_BINNED_ALL_LEVELS = 8,
       GS_FLAG_WIDE_RECORDS = 16, GS_FLAG_NO_SMALL_LEVELS = 32, GS_FLAG_MISPREDICT_LEVELS = 64,
       GS_FLAG_FRONTIER_EXCHANGE = 128, GS_FLAG_TRAJ_MULTI = 256 };

typedef struct gs_params {
  uint32_t push_fanout;         /* Config::gossip_push_fanout (gossip.rs:113) */
  uint32_t active_set_size;     /* Config::gossip_active_set_size, 1..32 */
  double rotation_probability;  /* Config::probability_of_rotation, [0,1] */
  uint64_t seed;                /* Philox key of the INIT/ROTATE/DECIDE/FAIL streams */
  int32_t device;               /* HIP device ordinal */
  uint32_t bfs_mode;            /* GS_BFS_* (results are identical in every mode) */
  uint32_t inbound_capacity;    /* per-(slot,node) inbound records per round; 0 = 64 */
  uint32_t flags;               /* GS_FLAG_PROFILE: time kernels with hipEvents; GS_FLAG_SPLIT_ROUND:
                                   gs_round launches the step kernels instead of the one-kernel
                                   workgroup round (same results; for A/B measurement);
                                   GS_FLAG_NARROW_WAVE_PATH: the one-kernel round sends in-degrees
                                   > 24 (not > 64) to its ordered single-lane consume, and the
                                   step-kernel round uses register paths for in-degree / entries
                                   <= 4 (not 16) and the wave consume for in-degree <= 8 (not 64)
                                   and the binned gather places records directly beyond 256
                                   per bin (same results; lets small test clusters cover every path);
                                   GS_FLAG_BINNED_ALL_LEVELS: GS_BFS_BINNED bins every level, not
                                   only levels with >= 2^17 frontier pairs (same results);
                                   GS_FLAG_WIDE_RECORDS: GS_BFS_BINNED keeps 8-byte push records
                                   even where 4-byte ones fit (same results);
                                   GS_FLAG_NO_SMALL_LEVELS: GS_BFS_BINNED / GS_BFS_MULTI run no level
                                   in their single-workgroup small-level kernels (every level
                                   through the grid-wide kernels; same results);
                                   GS_FLAG_MISPREDICT_LEVELS: GS_BFS_BINNED's predicted level loop
                                   inverts its binned/direct choice per level every other round
                                   (same results; a test of the misprediction path);
                                   GS_FLAG_FRONTIER_EXCHANGE: gs_create_part makes a frontier-exchange
                                   rank (gs_part_xbfs_*: it expands only its own frontier and
                                   exchanges each level's push records with their owners);
                                   GS_FLAG_TRAJ_MULTI: gs_create_traj may build its tables on the
                                   multi-source BFS (GS_BFS_MULTI, or AUTO beyond the workgroup
                                   engine); no effect on any other call */
} gs_params;

typedef struct gs_slot {
  uint32_t origin;               /* node id of the CRDS value owner (gossip_main.rs:360) */
  uint32_t min_ingress_nodes;    /* Config::min_ingress_nodes */
  double prune_stake_threshold;  /* Config::prune_stake_threshold */
} gs_slot;

/* Per slot, per recorded round: every integer the reference's per-round
 * statistics are built from (gossip_main.rs:480-563). f64 summaries are
 * computed on the host in the reference's order (gs_stats_*). */
typedef struct gs_round_summary {
  uint32_t visited;      /* n of RelativeMessageRedundancy: nodes reached incl. origin */
  uint32_t pushes;       /* pushes to non-failed peers (the m increments of gossip.rs:571) */
  uint32_t prunes;       /* prunees emitted by send_prunes (gossip.rs:684-687) */
  uint32_t stranded;     /* unreached, non-failed nodes (gossip.rs:329-345) */
  uint64_t hop_sum;      /* sum of hops over reached non-origin nodes */
  uint32_t hop_count;    /* number of reached non-origin nodes */
  uint32_t hop_min, hop_max, hop_med_lo, hop_med_hi; /* order statistics of those hops */
  uint32_t pad0;
  uint64_t stranded_stake_sum;
  uint64_t stranded_stake_min, stranded_stake_max, stranded_med_lo, stranded_med_hi;
} gs_round_summary;

typedef struct gs_engine gs_engine;

/* --- lifetime --------------------------------------------------------- */
int gs_create(const gs_params* params, const uint64_t* stakes, uint32_t n_nodes, uint32_t n_slots,
              gs_engine** out);
/* Several active-set trajectory tables in one engine (an active-set-size or
 * rotate-probability sweep as one engine): table t has its own ring size and rotation
 * probability and serves the next n_slots slots -- table 0 the slots [0, n0), table 1 the
 * next n1, ... fixed at create; the counts must sum to n_slots. params.active_set_size is
 * the capacity (1..32; row stride, push-mask width and LDS layout are sized by it, as
 * params.push_fanout sizes the per-slot fanouts) and every table's size is in [1, capacity];
 * params.rotation_probability is ignored. With gs_create_traj the seed is engine-wide: tables
 * draw the INIT / ROTATE / DECIDE streams a gs_create engine with that size and probability
 * draws, so each slot is bit-identical to its own per-value engine; the FAIL stream is shared.
 * gs_create_traj_seeds gives every table its own Philox key: table t draws INIT, ROTATE,
 * DECIDE and FAIL on seeds[t] (params.seed is ignored), so a slot of table t is bit-identical
 * to a gs_create engine with seed seeds[t], that size and that probability -- seed replicas,
 * and sweeps x replicas, run as one engine. seeds == NULL is exactly gs_create_traj; equal
 * seeds give the gs_create_traj engine at that seed (one array of fail ranks, the same memory
 * and kernels); otherwise every table holds its own fail ranks (4 B per node and table; the
 * multi-source BFS one more byte) and gs_read_failed reads the slot's own table's. Duplicate
 * (size, probability, seed) tables are allowed. Every rule below holds for both calls, and
 * seeds do not enter gs_traj_supported / gs_traj_multi_supported. gs_engine_traj_seeds reads
 * the keys back (GS_ERANGE and *n_traj when cap is too small): the engine's seed for every
 * table of an engine made another way. A prune
 * mask's bits are physical ring slots of the slot's own table. bfs_mode must be
 * GS_BFS_WORKGROUP or GS_BFS_AUTO (which resolves to WORKGROUP whatever the slot count), and
 * the network must fit the workgroup engine's LDS (gs_traj_supported, host arithmetic only:
 * returns 1 / 0, *fused = 1 if gs_round runs the one-kernel round at that capacity), else
 * GS_EINVAL; so are n_traj == 0, a table with n_slots == 0, a size of 0 or above the
 * capacity, a probability outside [0, 1]. n_traj == 1 is exactly gs_create with that size
 * and probability. Everything addressed by slot reads the slot's own table; the calls that
 * name an entry take the table (the _traj forms below; on an engine with several tables the
 * un-suffixed ones return GS_EINVAL). No reference interface: the reference builds one
 * Cluster per value (gossip_main.rs:775-797, 925-951).
 * With GS_FLAG_TRAJ_MULTI in params.flags the tables may also live on the multi-source BFS:
 * bfs_mode GS_BFS_MULTI builds a multi-source table engine at any size that BFS supports
 * (gs_traj_multi_supported: host arithmetic only, returns 1 / 0 for a network of n_nodes, an
 * engine of n_slots, a push-fanout capacity and a largest active-set size), GS_BFS_AUTO picks
 * WORKGROUP when gs_traj_supported and else MULTI, and LEVEL / BINNED / HYBRID stay GS_EINVAL.
 * Slot groups stay consecutive runs of slots, independent of the tables; a frontier entry
 * belongs to one table; the persistent and the launched level loop both run such engines, and
 * every slot stays bit-identical to its own per-value engine. Without the flag nothing
 * changes. */
typedef struct gs_traj {
  uint32_t active_set_size;      /* 1..params.active_set_size */
  double rotation_probability;   /* [0,1] */
  uint32_t n_slots;              /* this table serves the next n_slots slots */
} gs_traj;
int gs_create_traj(const gs_params* params, const uint64_t* stakes, uint32_t n_nodes, uint32_t n_slots,
                   const gs_traj* traj, uint32_t n_traj, gs_engine** out);
int gs_engine_traj(gs_engine* e, gs_traj* out, uint32_t cap, uint32_t* n_traj); /* reads the tables back */
int gs_create_traj_seeds(const gs_params* params, const uint64_t* stakes, uint32_t n_nodes, uint32_t n_slots,
                         const gs_traj* traj, uint32_t n_traj, const uint64_t* seeds /*[n_traj] or NULL*/,
                         gs_engine** out);
int gs_engine_traj_seeds(gs_engine* e, uint64_t* out, uint32_t cap, uint32_t* n_traj);
int gs_traj_supported(uint32_t n_nodes, uint32_t push_fanout, uint32_t max_active_set_size, int* fused);
int gs_traj_multi_supported(uint32_t n_nodes, uint32_t n_slots, uint32_t push_fanout, uint32_t max_active_set_size);
void gs_destroy(gs_engine* e);
const char* gs_last_error(void);
/* sha256 prefix (16 hex digits) of the device sources this library was built from; the
 * profiles under profiles/ are stamped with it (not a reference interface: measurement) */
const char* gs_kernel_hash(void);
int gs_device_count(int* n); /* HIP devices visible to this process (0 without a GPU) */
int gs_set_slots(gs_engine* e, const gs_slot* slots, uint32_t n_slots);
/* Per-slot Config::gossip_push_fanout: fanout[j] (n_slots values) is slot j's, each in
 * [1, params.push_fanout], else GS_EINVAL (gs_last_error names the slot) and nothing
 * changes. params.push_fanout is the engine's capacity: every buffer and kernel variant
 * stays sized by it, nothing is reallocated. NULL restores the uniform params.push_fanout.
 * Allowed whenever gs_set_slots is (before or after it; slot state is kept); takes effect at
 * the next gs_run_gossip / gs_round / gs_part_round / gs_part_xbfs_begin. An engine that never
 * receives the call, or whose values are all equal, runs the scalar-fanout kernels' path.
 * On node-range partition ranks the array is replicated state, like the slots: every rank
 * must be given the same values. gs_get_slot_fanouts reads the values back. */
int gs_set_slot_fanouts(gs_engine* e, const uint32_t* fanout /*[n_slots]*/);
int gs_get_slot_fanouts(gs_engine* e, uint32_t* out /*[n_slots]*/);
int gs_sync(gs_engine* e); /* waits for the stream and reports deferred device-side errors */

/* --- active sets: push_active_set.rs -------------------------------------- */
/* Node::initialize_gossip for every node (gossip.rs:805-813, gossip_main.rs:263-277). */
int gs_init_active_sets(gs_engine* e);
/* Overwrite / read one PushActiveSetEntry (push_active_set.rs:30) in FIFO order.
 * Setting an entry clears the prune state of its slots for every origin. */
int gs_set_active_set_entry(gs_engine* e, uint32_t node, uint32_t bucket, const uint32_t* peers, uint32_t len);
int gs_get_active_set_entry(gs_engine* e, uint32_t node, uint32_t bucket, uint32_t* peers, uint32_t cap,
                            uint32_t* len);

/* The same for table t of a gs_create_traj engine (t = 0 on any engine); setting an entry
 * clears the prune state of that table's slots only. */
int gs_set_active_set_entry_traj(gs_engine* e, uint32_t t, uint32_t node, uint32_t bucket, const uint32_t* peers,
                                 uint32_t len);
int gs_get_active_set_entry_traj(gs_engine* e, uint32_t t, uint32_t node, uint32_t bucket, uint32_t* peers,
                                 uint32_t cap, uint32_t* len);

/* --- the per-iteration steps: gossip.rs Cluster -------------------------- */
int gs_fail_nodes(gs_engine* e, const double* fraction_per_slot); /* Cluster::fail_nodes gossip.rs:756 */
int gs_run_gossip(gs_engine* e);                  /* Cluster::run_gossip gossip.rs:494 */
int gs_consume_messages(gs_engine* e);            /* Cluster::consume_messages gossip.rs:618 */
int gs_send_prunes(gs_engine* e);                 /* Cluster::send_prunes gossip.rs:657 */
int gs_prune_connections(gs_engine* e);           /* Cluster::prune_connections gossip.rs:701 */
int gs_chance_to_rotate(gs_engine* e, uint32_t round); /* Cluster::chance_to_rotate gossip.rs:739 */
int gs_record_round(gs_engine* e);                /* stats inserts gossip_main.rs:480-563 */
/* One iteration of gossip_main.rs:449-564 for every slot: run_gossip ->
 * consume -> send_prunes -> prune_connections -> chance_to_rotate(round) ->
 * (record != 0: the measured-round statistics). */
int gs_round(gs_engine* e, uint32_t round, int record);

/* --- readbacks (synchronise the engine stream) ----------------------------- */
int gs_read_hops(gs_engine* e, uint32_t slot, uint8_t* hops /*[n]*/); /* distances; 0xFF = u64::MAX */
/* orders (gossip.rs:601-607) as CSR by destination, each list in consume order
 * (hop, then id). off has n+1 entries. */
int gs_read_inbound(gs_engine* e, uint32_t slot, uint32_t* off, uint32_t* src, uint8_t* hop, size_t cap);
/* prunes of the last send_prunes (pruner, prunee) pairs sorted by (pruner, prunee). */
int gs_read_prunes(gs_engine* e, uint32_t slot, uint32_t* pruner, uint32_t* prunee, size_t cap, size_t* count);
/* ReceivedCache entry (received_cache.rs:13-17) of `node` for the slot's origin, keys sorted. */
int gs_read_cache(gs_engine* e, uint32_t slot, uint32_t node, uint32_t* num_upserts, uint32_t* keys,
                  uint32_t* scores, uint32_t cap, uint32_t* len);
/* Prune state of `node`'s entry for the slot's origin, bit i = i-th peer in FIFO order pruned. */
int gs_read_pruned(gs_engine* e, uint32_t slot, uint32_t node, uint32_t* fifo_mask);
/* Bulk forms for parity diffing: every entry in FIFO order (peers[(node*25+k)*active_set_size + i],
 * len[node*25+k]); every node's cache for the slot (keys sorted, 96 per node); every node's FIFO prune mask. */
int gs_read_active_sets(gs_engine* e, uint32_t* peers, uint8_t* len);
/* table t's entries, with a row stride of that table's own size */
int gs_read_active_sets_traj(gs_engine* e, uint32_t t, uint32_t* peers, uint8_t* len);
int gs_read_caches(gs_engine* e, uint32_t slot, uint32_t* num_upserts, uint32_t* len, uint32_t* keys,
                   uint32_t* scores);
int gs_read_pruned_all(gs_engine* e, uint32_t slot, uint32_t* fifo_mask);
/* this round's egress/ingress/prune-sent counts (gossip.rs:185-189); egress of an
 * unreached node reads 0 */
int gs_read_counters(gs_engine* e, uint32_t slot, uint32_t* egress, uint32_t* ingress, uint32_t* prune_sent);
/* recorded rounds so far: out[r * n_slots + slot] */
int gs_read_round_summaries(gs_engine* e, gs_round_summary* out, size_t cap, size_t* count);
/* measured-round accumulators: message trackers (gossip_stats.rs:359-461), times
 * stranded per node (gossip_stats.rs:849) and the hop histogram (raw_hop_collection) */
int gs_read_accumulators(gs_engine* e, uint32_t slot, uint64_t* egress, uint64_t* ingress, uint64_t* prunes,
                         uint32_t* stranded_times, uint64_t* hop_hist /*[256]*/);
int gs_read_failed(gs_engine* e, uint32_t slot, uint8_t* failed /*[n]*/);
/* --- cluster load view: per-node message load summed over every slot ---------
 * The trackers above are per slot, as the reference's are per origin (gossip_stats.rs:359-461:
 * one Cluster is one origin). When the slots are the origins of one configuration ("all
 * origins"), what a node sends and receives in a round is the sum over the slots -- the load
 * the push/prune protocol exists to bound. With eg_j / in_j / pr_j the arrays gs_read_counters
 * returns for slot j (egress of an unreached node reads 0) and h_j gs_read_hops', a recorded
 * round r has, per node v:
 *   E_r[v] = sum_j eg_j[v]   I_r[v] = sum_j in_j[v]   P_r[v] = sum_j pr_j[v]
 *   D_r[v] = #{j : 1 <= h_j[v] <= 254}  (deliveries: slots that reached v, v not their origin)
 *   H_r[v] = the sum of those h_j[v]
 * gs_read_cluster_load returns, over the recorded rounds since the last gs_set_slots (the
 * accumulators' rule), the totals of E, I, P, D, H and the peaks max_r E_r[v], max_r I_r[v];
 * gs_read_cluster_rounds one gs_cluster_round per recorded round, entry r being the round of
 * gs_read_round_summaries' row r: the sums over v of E_r, I_r, P_r, D_r, the largest E_r[v]
 * and I_r[v] with their nodes (the smallest id among equals) and the nodes with E_r[v] > 0.
 * All integer sums and maxima: exact, whatever the order of the reduction.
 * The view sums EVERY slot of the engine, whatever its table, fanout or threshold: it means
 * "load" only when the slots are origins of one configuration; gs_cluster_enable_groups
 * (below) sums per group of slots, with a weight per slot.
 * gs_cluster_enable(on != 0) allocates the view (about 68 B per node and 56 B per recorded
 * round held on the device, counted in gs_engine_info's bytes and gs_engine_memory's
 * other_bytes) and zeroes it; it is allowed whenever gs_set_slots is, before or after it;
 * enabling an enabled view is a no-op; on == 0 frees it. gs_set_slots zeroes it. Rounds
 * recorded before the view was enabled read as all-zero entries. While enabled, every
 * recorded round (gs_round with record != 0 on every path, gs_record_round) runs the
 * reduction as two launches of their own behind the round's last kernel (kernel family
 * "cluster"); a round that is not recorded launches nothing, and an engine that never enables
 * the view allocates and launches nothing. The reads without an enabled view, and
 * gs_cluster_enable on a node-range partition rank (gs_create_part: the ranks' per-round sums
 * would need an exchange), return GS_ESTATE; a geometry whose per-round sums could pass u32
 * (n_slots x max(255, inbound capacity) >= 2^32) GS_ERANGE. No reference interface. */
typedef struct gs_cluster_round {
  uint64_t pushes, ingress, prunes, delivered;
  uint32_t egress_max, egress_max_node, ingress_max, ingress_max_node;
  uint32_t senders, pad0;
} gs_cluster_round;
int gs_cluster_enable(gs_engine* e, int on);
int gs_read_cluster_load(gs_engine* e, uint64_t* egress, uint64_t* ingress, uint64_t* prunes,
                         uint64_t* delivered, uint64_t* hop_sum,        /* [n] each, NULL = skip */
                         uint32_t* egress_peak, uint32_t* ingress_peak);
/* *count = recorded rounds so far; GS_ERANGE when cap is smaller */
int gs_read_cluster_rounds(gs_engine* e, gs_cluster_round* out, size_t cap, size_t* count);
/* --- the view per slot group, with a weight per slot ---------------------------
 * The slots are cut into n_groups groups of consecutive slots (group g: group_slots[g] slots
 * behind those of the groups before it, as the trajectory tables are laid out) and slot j
 * counts weights[j] times (u32; 0 excludes the slot; NULL = 1 each). Per group g:
 *   E_r^g[v] = sum_{j in g} w_j eg_j[v], and I, P likewise;
 *   D_r^g[v] = sum_{j in g} w_j [1 <= h_j[v] <= 254];  H_r^g[v] = sum of w_j h_j[v] over those j.
 * Every group keeps what the ungrouped view keeps: totals, peaks and one gs_cluster_round per
 * recorded round. group_slots == NULL with n_groups == 0: one group per trajectory table
 * (gs_create_traj[_seeds]; one group on an engine made another way).
 * gs_cluster_enable_groups is allowed whenever gs_cluster_enable is; allocation is all or nothing
 * (GS_ENOMEM): about 68 B per node and 56 B per held round, each times n_groups, plus 12 B per
 * slot chunk and 4 B per slot, counted like the ungrouped view's. GS_EINVAL (the message names
 * the argument): counts that do not sum to n_slots, an empty group, n_groups > n_slots, a null
 * group_slots with n_groups != 0. GS_ERANGE (the message names the group): a group whose
 * (sum of weights) x max(255, inbound capacity) >= 2^32 -- the per-round sums stay u32 -- or
 * more than 65,535 groups or slot chunks. GS_ESTATE: a partition rank; a view with another
 * grouping or other weights is enabled (disable it first: gs_cluster_enable(e, 0) frees either
 * kind); enabling the identical grouping again is a no-op. A view of one group and unit weights
 * and gs_cluster_enable's are the same grouping: either call is a no-op after the other, and
 * gs_cluster_enable(e, 1) over any other grouped view is GS_ESTATE. A refused call leaves the
 * engine as it was. gs_set_slots zeroes every group; rounds recorded before enabling read as
 * zero entries in every group. The round's reduction stays two launches, whatever n_groups.
 * gs_cluster_groups reads the grouping back (*n_groups is set also when cap is too small:
 * GS_ERANGE; weights [n_slots] or NULL); for gs_cluster_enable's view: 1 group, unit weights.
 * The _group reads take the un-suffixed reads' arguments after g (g >= n_groups: GS_EINVAL);
 * the un-suffixed reads return group 0 of a one-group view and GS_EINVAL when there are more. */
int gs_cluster_enable_groups(gs_engine* e, const uint32_t* group_slots, uint32_t n_groups,
                             const uint32_t* weights /*[n_slots] or NULL = 1*/);
int gs_cluster_groups(gs_engine* e, uint32_t* group_slots, uint32_t cap, uint32_t* n_groups,
                      uint32_t* weights /*[n_slots] or NULL*/);
int gs_read_cluster_load_group(gs_engine* e, uint32_t g, uint64_t* egress, uint64_t* ingress, uint64_t* prunes,
                               uint64_t* delivered, uint64_t* hop_sum, uint32_t* egress_peak,
                               uint32_t* ingress_peak);
int gs_read_cluster_rounds_group(gs_engine* e, uint32_t g, gs_cluster_round* out, size_t cap, size_t* count);
/* Cluster::mst (gossip.rs:580-591): parent[v] = the node that first discovered v in the
 * reference's FIFO queue order, UINT32_MAX for the origin and unreached nodes (debug
 * readback after gs_run_gossip, n <= 262,144). */
int gs_read_mst(gs_engine* e, uint32_t slot, uint32_t* parent /*[n]*/);
/* GS_FLAG_PROFILE: summed device time of a kernel family ("bfs", "consume",
 * "rotate", "stats", "cluster": the cluster load view's two launches per recorded round)
 * since the last reset, and its launch count. */
int gs_kernel_time(gs_engine* e, const char* family, double* ms, uint64_t* launches);
int gs_kernel_time_reset(gs_engine* e);
int gs_engine_info(gs_engine* e, uint32_t* n_nodes, uint32_t* n_slots, uint32_t* bfs_mode, uint64_t* device_bytes);
/* device_bytes split: per-(slot, node) state (hops, in-degrees, caches, counters,
 * accumulators, record pools; a partition rank's own nodes) and everything else (rows,
 * masks, per-node and per-slot tables, BFS queues). */
int gs_engine_memory(gs_engine* e, uint64_t* pair_bytes, uint64_t* other_bytes);
/* 1 if gs_round runs the one-kernel workgroup round (BFS, consume, prune and
 * statistics per slot in one workgroup), 0 if it launches the step kernels. */
int gs_engine_round_kind(gs_engine* e, uint32_t* fused);
/* Round split (GS_ROUND_SPLIT, default on; =0 off): gs_round on a one-kernel engine with one
 * trajectory table, no cluster view, no partition and at least twice as many slots as round
 * workgroups fit on the device launches the slots as two groups on two streams, so one group's
 * workgroups fill the compute units the other's launch leaves idle while it ends. Results are
 * the single-stream round's, bit for bit. out[0] 1 if gs_round splits now, out[1] / out[2] the
 * slots of the two groups (zeros when off). n >= 3. */
int gs_engine_round_split(gs_engine* e, uint32_t* out, size_t n);
/* Geometry of the multi-source / hybrid BFS (diagnostics; not a reference interface): out[0]
 * frontier entries (multi) or nodes (hybrid) per expand slice, out[1] coarse destination bins,
 * out[2] fine bins, out[3] slots per slot group, out[4] slot groups; with n >= 6, out[5] the
 * workgroups of the persistent BFS launch (0: the launched level loop runs). n >= 5; zeros in
 * other modes. */
int gs_engine_bfs_geometry(gs_engine* e, uint32_t* out, size_t n);

/* --- node-range partition ------------------------------
 * K engines, one per rank/GPU, created with gs_create_part on the same stakes, params
 * (bfs_mode GS_BFS_MULTI or AUTO), slots and seed. Rank r owns the node ids
 * [node_lo, node_hi) (gs_part_sizes): K contiguous ranges of whole 1,024-id bins of
 * C = ceil(n / K) rounded up to 1,024; every rank must own a node ((K - 1) * C < n, else
 * gs_create_part fails with GS_EINVAL on the empty ranks -- check before creating).
 * K = 1 gives one rank owning every node (the exchange calls work; a one-rank group). 
 * Replicated on every rank: active sets, prune masks, failed flags (the same rotations,
 * failures and prune bits are applied everywhere). Kept for owned nodes only: every
 * per-(slot, node) array -- hops, in-degrees, received caches, round counters,
 * accumulators -- i.e. S x (node_hi - node_lo) pairs. Each rank runs the whole BFS over
 * its replicated tables (no exchange per level) and gathers, consumes and prunes for
 * its own nodes. One iteration of gossip_main.rs:449-564 is:
 *   gs_part_round(round, record, &n)        run_gossip + consume + send_prunes; n prune records
 *   ALL-GATHER the n's, then prune_connections by ONE of (every rank picks the same):
 *     records: ALL-GATHER the ranks' records (gs_part_prunes_out, n x 2 u32 words: slot *
 *       n_nodes + prunee, ring-slot bits) -> gs_part_prunes_in(all records); only while
 *       every n <= record_cap (gs_part_exchange_sizes) and the records are the smaller form;
 *     dense: gs_part_prunes_dense_out (dense_words u32 = [n_nodes][n_slots] ring-slot bits)
 *       -> SUM ALL-REDUCE (the ranks' bits are disjoint: SUM = OR) -> gs_part_prunes_dense_in;
 *   gs_chance_to_rotate(round);
 *   if recorded: gs_part_stats_out -> SUM over ranks -> gs_part_stats_in.
 * The exchanges are the caller's: RCCL on device buffers over xGMI, or host buffers
 * (dst_device / src_device select which). Readbacks of per-pair arrays fill the owned
 * nodes (hops 0xFF, counters 0 and empty caches elsewhere); gs_round and the step-wise
 * calls (gs_run_gossip ...) return GS_ESTATE on a partition rank.
 * Replaces: the same loop as gs_round over one engine (results identical on owned nodes). */
int gs_create_part(const gs_params* params, const uint64_t* stakes, uint32_t n_nodes, uint32_t n_slots,
                   uint32_t rank, uint32_t nranks, gs_engine** out);
int gs_part_sizes(gs_engine* e, size_t* stats_words, uint32_t* node_lo, uint32_t* node_hi);
int gs_part_round(gs_engine* e, uint32_t round, int record, uint32_t* n_records);
int gs_part_prunes_out(gs_engine* e, void* dst, int dst_device);                 /* [n_records][2] u32 */
int gs_part_prunes_in(gs_engine* e, const void* src, size_t n_records, int src_device);
int gs_part_exchange_sizes(gs_engine* e, size_t* record_cap, size_t* dense_words);
int gs_part_prunes_dense_out(gs_engine* e, void* dst, int dst_device);           /* [n_nodes][n_slots] u32 */
int gs_part_prunes_dense_in(gs_engine* e, const void* src, int src_device);
/* Frontier exchange (params.flags GS_FLAG_FRONTIER_EXCHANGE; SURVEY 8(e), the north star's
 * "node-range partition with RCCL frontier exchange"). Ranks own whole coarse destination bins
 * (C = ceil(n / K) rounded up to max(1,024, the multi BFS's coarse bin)); each rank expands
 * ONLY the frontier entries of its own nodes, and each level's push records go to the rank
 * owning their destination, which applies them (first arrivals, pool records, its own
 * next-level entries). For each slot group g < n_groups, the BFS is
 *   gs_part_xbfs_begin(g, &n)                        seeds the group's own origins; n own entries
 *   level d = 0, 1, ... while the SUM of n over ranks > 0:
 *     gs_part_xbfs_expand(d, words_to[K])            expand own entries, pack per owner rank
 *     ALL-TO-ALL the K counts, then gs_part_xbfs_send(buf) -> ALL-TO-ALL (split by words_to /
 *       words_from, u64 words: per message the owner's bin counts, then the records)
 *     gs_part_xbfs_apply(d, recv, words_from[K], &n)  apply what every rank pushed here
 *   gs_part_xbfs_end(record)                         gather of the group's own nodes (inbound rows)
 * then gs_part_xround_finish(round, record, &n_records) (consume_messages of every group's rows,
 * send_prunes of own pruners; with GS_MV_FUSED=1 the consume runs fused in xbfs_end instead)
 * in place of gs_part_round; the prune and statistics exchanges follow as above. */
int gs_part_xbfs_groups(gs_engine* e, uint32_t* n_groups);
int gs_part_xbfs_begin(gs_engine* e, uint32_t group, uint32_t* n_local);
int gs_part_xbfs_expand(gs_engine* e, uint32_t level, uint64_t* words_to /*[K]*/);
int gs_part_xbfs_send(gs_engine* e, void* dst, int dst_device);
int gs_part_xbfs_apply(gs_engine* e, uint32_t level, const void* src, const uint64_t* words_from /*[K]*/,
                       int src_device, uint32_t* n_local);
int gs_part_xbfs_end(gs_engine* e, int record);
/* The same level loop without a host wait per level (round 6): every rank's message to rank q
 * goes to the fixed slot [q * cap_words, (q + 1) * cap_words) of `send` (device memory, K
 * slots), so the all-to-all moves K equal slots and no size reaches the host. The caller
 * runs the predicted number of levels (the previous round's, agreed by all ranks; levels
 * past the BFS's end are no-ops), enqueues the collective on the engine's stream
 * (gs_stream), then calls gs_part_xbfs_async_status once: n_local = this rank's entries of
 * the next level (all ranks 0: the BFS is over, else continue with gs_part_xbfs_expand /
 * _apply from that level), overflow = 1 if a message outgrew its slot (then every rank
 * redoes the group: gs_part_xbfs_begin again), words_log [levels][K] = the words each
 * level sent to each rank (the next round's slot sizes). cap_words must hold every rank's
 * bin headers. Replaces the per-level size exchange of gossip.rs:511-609's partitioned
 * form; no reference interface. */
int gs_part_xbfs_expand_async(gs_engine* e, uint32_t level, uint64_t cap_words, void* send);
int gs_part_xbfs_apply_async(gs_engine* e, uint32_t level, const void* recv, uint64_t cap_words);
int gs_part_xbfs_async_status(gs_engine* e, uint32_t* n_local, uint32_t* overflow, uint64_t* words_log,
                              size_t log_levels);
/* The engine's HIP stream (hipStream_t), e.g. to enqueue a collective behind its kernels. */
int gs_stream(gs_engine* e, void** stream);
int gs_part_xround_finish(gs_engine* e, uint32_t round, int record, uint32_t* n_records);
int gs_part_stats_out(gs_engine* e, void* dst, int dst_device);          /* [S][5 + 256 + W] u64 */
int gs_part_stats_in(gs_engine* e, const void* src, int src_device);

/* --- host-side statistics (gossip_stats.rs), f64 in the reference's order --- */
typedef struct gs_hops_stat { double mean, median; uint64_t max, min; } gs_hops_stat;
typedef struct gs_stat4 { double mean, median, max, min; } gs_stat4;
/* HopsStat::new (gossip_stats.rs:47-98) over raw distances (u64::MAX = unreached). */
int gs_hops_stat_new(const uint64_t* hops, size_t n, gs_hops_stat* out);
/* StatCollection::calculate_stats (gossip_stats.rs:266-295). */
int gs_stat_collection_calculate(const double* values, size_t n, gs_stat4* out);

/* --- whole simulations: gossip_main.rs run_simulation ---------------------- */
typedef struct gs_sim_config {  /* gossip.rs Config (gossip.rs:111-133) */
  uint32_t push_fanout, active_set_size, iterations, warm_up_rounds;
  uint32_t min_ingress_nodes, when_to_fail;
  double rotation_probability, prune_stake_threshold, fraction_to_fail;
  uint64_t num_buckets_stranded, num_buckets_message, num_buckets_hops;
  int32_t test_type;  /* 0 none, 1 active-set-size, 2 min-ingress-nodes, 3 push-fanout,
                         4 prune-stake-threshold, 5 fail-nodes, 6 origin-rank, 7 rotate-probability */
  uint64_t seed;
  int32_t device;
  uint32_t bfs_mode;
} gs_sim_config;

typedef struct gs_sim_result gs_sim_result;
/* Runs n_sims simulations that share one active-set trajectory as slots of one
 * engine; sims differ only in origin_rank / min_ingress / threshold / fraction (and, with
 * gs_run_simulations_fanouts, push fanout). */
int gs_run_simulations(const gs_sim_config* cfg, const uint64_t* stakes, uint32_t n_nodes, uint32_t n_sims,
                       const uint32_t* origin_ranks, const uint32_t* min_ingress, const double* thresholds,
                       const double* fractions, gs_sim_result** out);
/* The same with a push fanout per sim (a push-fanout sweep at one active-set size as one
 * engine): fanouts == NULL is exactly gs_run_simulations (every sim takes cfg->push_fanout);
 * otherwise the engine is created with push_fanout = max(fanouts) and the per-slot values
 * are set (gs_set_slot_fanouts) before gs_init_active_sets. */
int gs_run_simulations_fanouts(const gs_sim_config* cfg, const uint64_t* stakes, uint32_t n_nodes, uint32_t n_sims,
                               const uint32_t* origin_ranks, const uint32_t* min_ingress, const double* thresholds,
                               const double* fractions, const uint32_t* fanouts, gs_sim_result** out);
/* The same with an active-set size and a rotation probability per sim (an active-set-size or
 * rotate-probability sweep as one engine): one value per sim, or NULL for cfg's. The sims are
 * grouped by (size, probability) into the tables of one gs_create_traj engine -- equal pairs
 * need not be adjacent -- and the results come back in sim order. Both NULL is exactly
 * gs_run_simulations_fanouts; one distinct pair is that call at the pair's values. With
 * cfg->bfs_mode == GS_BFS_MULTI and several pairs the call sets GS_FLAG_TRAJ_MULTI itself and
 * the engine is a multi-source table engine; any other mode behaves as gs_create_traj does. */
int gs_run_simulations_traj(const gs_sim_config* cfg, const uint64_t* stakes, uint32_t n_nodes, uint32_t n_sims,
                            const uint32_t* origin_ranks, const uint32_t* min_ingress, const double* thresholds,
                            const double* fractions, const uint32_t* fanouts, const uint32_t* active_set_sizes,
                            const double* rotation_probabilities, gs_sim_result** out);
/* The same with a Philox seed per sim as well (seed replicas, and sweeps x replicas, as one
 * engine): seeds == NULL is exactly gs_run_simulations_traj. Otherwise the sims are grouped by
 * (size, probability, seed) into the tables of one gs_create_traj_seeds engine, permuted into
 * table order and back; cfg->seed is unused. One distinct triple is gs_run_simulations_fanouts
 * at that triple (cfg->seed replaced by the seed). */
int gs_run_simulations_seeds(const gs_sim_config* cfg, const uint64_t* stakes, uint32_t n_nodes, uint32_t n_sims,
                             const uint32_t* origin_ranks, const uint32_t* min_ingress, const double* thresholds,
                             const double* fractions, const uint32_t* fanouts, const uint32_t* active_set_sizes,
                             const double* rotation_probabilities, const uint64_t* seeds /*per sim or NULL*/,
                             gs_sim_result** out);
/* The same with the cluster load view: cluster == 0 is exactly gs_run_simulations_seeds;
 * otherwise the engine's view is enabled (gs_cluster_enable) before gs_init_active_sets, and
 * the result also answers gs_result_u64 for -- the same arrays under any valid sim, in node id
 * order -- "cluster_egress", "cluster_ingress", "cluster_prunes", "cluster_delivered",
 * "cluster_hop_sum", "cluster_egress_peak", "cluster_ingress_peak" ([n] each) and, one value
 * per measured round, "cluster_round_pushes", "cluster_round_egress_max",
 * "cluster_round_egress_max_node", "cluster_round_ingress_max", "cluster_round_ingress_max_node",
 * "cluster_round_senders". Every other name reads what it reads with cluster == 0. */
int gs_run_simulations_cluster(const gs_sim_config* cfg, const uint64_t* stakes, uint32_t n_nodes, uint32_t n_sims,
                               const uint32_t* origin_ranks, const uint32_t* min_ingress, const double* thresholds,
                               const double* fractions, const uint32_t* fanouts, const uint32_t* active_set_sizes,
                               const double* rotation_probabilities, const uint64_t* seeds /*per sim or NULL*/,
                               int cluster, gs_sim_result** out);
/* The same with the view grouped by trajectory table (gs_cluster_enable_groups with one group per
 * table; the sims of one (size, probability, seed) are one table, so one group) and a weight per
 * sim (NULL = 1), permuted into table order with the sims. The cluster_* names under a sim answer
 * with the arrays of that sim's own group. */
int gs_run_simulations_cluster_tables(const gs_sim_config* cfg, const uint64_t* stakes, uint32_t n_nodes,
                                      uint32_t n_sims, const uint32_t* origin_ranks, const uint32_t* min_ingress,
                                      const double* thresholds, const double* fractions, const uint32_t* fanouts,
                                      const uint32_t* active_set_sizes, const double* rotation_probabilities,
                                      const uint64_t* seeds /*per sim or NULL*/,
                                      const uint32_t* weights /*per sim or NULL*/, gs_sim_result** out);
void gs_result_free(gs_sim_result* r);
/* Named arrays of a finished sim (same names as the oracle): e.g. "coverage",
 * "rmr", "coverage_stats", "stranded", "hops_hist" ... Returns the element
 * count (copies min(count, cap)); SIZE_MAX for an unknown name. */
size_t gs_result_f64(const gs_sim_result* r, uint32_t sim, const char* name, double* out, size_t cap);
size_t gs_result_u64(const gs_sim_result* r, uint32_t sim, const char* name, uint64_t* out, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* GOSSIP_HIP_H */
