// gossip_sim_main.cpp -- the `gossip-sim` driver (gossip_main.rs:53-981) on the HIP
// engine, plus `gossip-sim write-accounts` (write_accounts_main.rs:18-128).
//
// Same flags, defaults, validation and test-type sweeps as the reference. A sweep's
// simulations that share one active-set trajectory (no-test, origin-rank,
// min-ingress-nodes, prune-stake-threshold, fail-nodes) run as slots of ONE engine. So do
// the sims of a push-fanout sweep that share an active-set size (the fanout is a per-slot
// value of the engine; the reference raises a sim's set size to its fanout, which splits the
// sweep into one engine per size). The test types that change the trajectory itself
// (active-set-size, rotate-probability) give each value its own engine. --engine-plan FILE
// writes the engines of a run. --trials K repeats every simulation at the seeds --seed ..
// --seed + K - 1 (value-major, trial-minor; each repeat is a simulation of its own): one engine per
// (trajectory value, seed), or with --batch-sweeps one engine per device whose tables carry their
// own seeds. With --gpus K the simulations are dealt over K devices,
// one host thread and engine per device (results do not depend on the split: the
// Philox contract makes every slot a pure function of its own parameters).
//
// Offline stand-ins for the reference's network services: accounts come from the
// stake YAML (--accounts-from-yaml --account-file) or the deterministic synthetic
// network (--synthetic N) instead of an RPC pull; --influx other than `n` is refused.
// --save-results / --replay-results keep the named result arrays of a run in a text
// file and print the report from it again without a GPU. --cluster-load PATH runs every
// engine with its cluster load view on and writes each node's load summed over all origins;
// --cluster-load-by-config PATH groups the view by trajectory table and writes it per table.
#include <algorithm>
#include <cerrno>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <chrono>
#include <thread>
#include <tuple>
#include <vector>

#include "../../include/gossip_hip.h"
#include "gs_io.h"
#include "gs_report.h"

namespace {

const char* TMAIN = "gossip_sim";

const char* F64_NAMES[] = {"coverage", "rmr", "branching", "hop_mean", "hop_median", "coverage_stats", "rmr_stats",
                           "branching_stats", "aggregate_hops", "ldh", "stranded", "stranded_round_mean",
                           "stranded_round_median"};
const char* U64_NAMES[] = {"origin", "hop_max", "hop_min", "aggregate_hops", "ldh", "stranded", "stranded_times",
                           "stranded_round_count", "stranded_round_max", "stranded_round_min", "hops_hist",
                           "stranded_hist", "egress_hist", "ingress_hist", "prune_hist", "egress_cpb",
                           "validator_hist", "hist_errors", "failed_count", "rmr_m", "rmr_n"};
// --cluster-load: the totals of the cluster load view (additive across engines; peaks and
// per-round lines are not, and are not kept)
const char* CLUSTER_NAMES[] = {"cluster_egress", "cluster_ingress", "cluster_prunes", "cluster_delivered",
                               "cluster_hop_sum"};

// --cluster-load-by-config: the totals of one table's group are kept under the table's first
// simulation, with the table's index within its engine under this name
const char* CLUSTER_TABLE = "cluster_table";

[[noreturn]] void die(int code, const std::string& msg) {
  std::fprintf(stderr, "error: %s\n", msg.c_str());
  std::exit(code);
}

bool parse_u64(const std::string& s, uint64_t& out) {
  if (s.empty() || s.find_first_not_of("0123456789") != std::string::npos) return false;
  errno = 0;
  char* end = nullptr;
  out = std::strtoull(s.c_str(), &end, 10);
  return errno == 0 && end && *end == 0;
}
bool parse_f64(const std::string& s, double& out) {
  if (s.empty()) return false;
  char* end = nullptr;
  out = std::strtod(s.c_str(), &end);
  return end && *end == 0;
}

struct Cli {
  std::string account_file, url = "https://api.mainnet-beta.solana.com", influx = "n", test_type_s;
  bool accounts_from_yaml = false, filter_zero = false, print_stats = false;
  uint64_t fanout = 6, asz = 12, iterations = 1, min_ingress = 2, nb_stranded = 10, nb_message = 5, nb_hops = 15;
  std::vector<uint64_t> origin_ranks = {1};
  std::string p_s = ".013333", thr_s = ".15", num_sims_s = "1", step_s = "1", frac_s = "0.1";
  uint64_t when_to_fail = 0, warm_up = 200;
  // engine / offline extensions
  uint64_t synthetic = 0, seed = 0x5EED0003ull, gpus = 1, bfs_mode = GS_BFS_AUTO;
  std::string save_results, replay_results, engine_plan;
  std::string cluster_load;   // per-node load summed over every simulation of every engine
  std::string cluster_by_config;  // per-node load per (engine, trajectory table)
  std::string influx_file;  // offline Influx line protocol (gs_influx.cpp)
  uint64_t influx_time_base = 0;
  bool batch_sweeps = false;  // an active-set-size / rotate-probability / push-fanout sweep as one engine per device
  uint64_t trials = 1;        // every simulation repeated at seeds seed .. seed + trials - 1
};

void usage() {
  std::puts(
      "gossip-sim: push-propagation gossip simulator (MI355X HIP engine)\n"
      "  --account-file PATH            yaml of accounts to read (with --accounts-from-yaml)\n"
      "  --accounts-from-yaml           read pubkey: stake pairs from --account-file\n"
      "  -f, --filter-zero-staked-nodes drop zero-staked nodes\n"
      "  --push-fanout N [6]  --active-set-size N [12]  --iterations N [1]\n"
      "  --origin-rank N... [1]  -p, --rotation-probability P [.013333]\n"
      "  --min-ingress-nodes N [2]  --prune-stake-threshold T [.15]\n"
      "  --num-buckets-stranded N [10]  --num-buckets-message N [5]  --num-buckets-hops N [15]\n"
      "  --test-type active-set-size|push-fanout|min-ingress-nodes|prune-stake-threshold|origin-rank|\n"
      "              rotate-probability|fail-nodes\n"
      "  --num-simulations N [1]  --step-size X [1]  --fraction-to-fail F [0.1]  --when-to-fail N [0]\n"
      "  --warm-up-rounds N [200]  --influx n  --print-stats  --url URL (no RPC offline)\n"
      "engine / offline options:\n"
      "  --synthetic N        the deterministic synthetic power-law network of N nodes instead of RPC\n"
      "  --seed S [0x5EED0003] --gpus K [1] --bfs-mode 0..5 [0 = auto; 1 workgroup, 2 level, 3 binned, 4 multi, 5 hybrid]\n"
      "  --save-results PATH  --replay-results PATH (print the report of a saved run, no GPU)\n"
      "  --cluster-load PATH  run every engine with its cluster load view and write one line per node in id order:\n"
      "                       pubkey,stake,egress,ingress,prunes,delivered,hop_sum -- the measured rounds' totals\n"
      "                       summed over every simulation (origin) of every engine of the run; --save-results then\n"
      "                       keeps these totals, and --replay-results with --cluster-load rewrites the file\n"
      "  --cluster-load-by-config PATH  run every engine with its view grouped by trajectory table (the simulations\n"
      "                       of one active-set size, rotation probability and seed; one table per engine without\n"
      "                       --batch-sweeps) and write one line per engine of the plan, table and node:\n"
      "                       engine,table,pubkey,stake,egress,ingress,prunes,delivered,hop_sum -- --save-results keeps\n"
      "                       each table's totals under its first simulation, and --replay-results rewrites the file\n"
      "  --engine-plan PATH   write one line per engine: device, simulations, active-set size, fanouts\n"
      "  --batch-sweeps       run an active-set-size, rotate-probability or push-fanout sweep as ONE engine per\n"
      "                       device (an active-set table per value) instead of one engine per value; a plan\n"
      "                       line then lists active-set-size, fanouts and rotation-probability per simulation.\n"
      "                       Networks beyond the workgroup engine (about 16,000 nodes) fall back to one engine\n"
      "                       per value, unless --bfs-mode 4 is given: then the tables live on the multi-source\n"
      "                       BFS at any node count it supports (one engine per device)\n"
      "  --trials K [1]       repeat every simulation at the seeds --seed, --seed + 1, .. --seed + K - 1 (value-major,\n"
      "                       trial-minor; each repeat is its own simulation in the report and in --save-results):\n"
      "                       one engine per (trajectory value, seed), or with --batch-sweeps one engine per device\n"
      "                       (a table per value and seed) under the same network limits; plan lines gain `seeds`\n"
      "  --influx-file PATH   write the Influx series (influx_db.rs) as line protocol to PATH\n"
      "  --influx-time-base NS  reproducible Influx timestamps NS + 1000 k (default: wall clock)\n"
      "gossip-sim write-accounts --account-file PATH --synthetic N [--num-nodes K] [--zero-stakes] [-f]");
}

Cli parse(int argc, char** argv) {
  Cli c;
  std::vector<std::string> args;  // "--flag=value" split into two tokens
  for (int i = 1; i < argc; ++i) {
    const std::string x = argv[i];
    const size_t eq = x.find('=');
    if (x.rfind("--", 0) == 0 && eq != std::string::npos) {
      args.push_back(x.substr(0, eq));
      args.push_back(x.substr(eq + 1));
    } else {
      args.push_back(x);
    }
  }
  const int n = (int)args.size();
  auto need = [&](int& i) -> std::string {
    if (i + 1 >= n) die(2, "missing value for " + args[i]);
    return args[++i];
  };
  auto u64 = [&](int& i, uint64_t& dst) {
    const std::string flag = args[i], v = need(i);
    if (!parse_u64(v, dst)) die(2, "invalid value '" + v + "' for " + flag);
  };
  for (int i = 0; i < n; ++i) {
    const std::string a = args[i];
    if (a == "-h" || a == "--help") { usage(); std::exit(0); }
    else if (a == "--url") c.url = need(i);
    else if (a == "--account-file") c.account_file = need(i);
    else if (a == "--accounts-from-yaml") c.accounts_from_yaml = true;
    else if (a == "-f" || a == "--filter-zero-staked-nodes") c.filter_zero = true;
    else if (a == "--push-fanout") u64(i, c.fanout);
    else if (a == "--active-set-size") u64(i, c.asz);
    else if (a == "--iterations") u64(i, c.iterations);
    else if (a == "--origin-rank") {
      c.origin_ranks.clear();
      while (i + 1 < n && args[i + 1][0] != '-') {
        uint64_t r = 0;
        if (!parse_u64(args[i + 1], r)) die(2, "invalid value '" + args[i + 1] + "' for --origin-rank");
        c.origin_ranks.push_back(r);
        ++i;
      }
      if (c.origin_ranks.empty()) die(2, "missing value for --origin-rank");
    } else if (a == "-p" || a == "--rotation-probability") c.p_s = need(i);
    else if (a == "--min-ingress-nodes") u64(i, c.min_ingress);
    else if (a == "--prune-stake-threshold") c.thr_s = need(i);
    else if (a == "--num-buckets-stranded") u64(i, c.nb_stranded);
    else if (a == "--num-buckets-message") u64(i, c.nb_message);
    else if (a == "--num-buckets-hops") u64(i, c.nb_hops);
    else if (a == "--test-type") c.test_type_s = need(i);
    else if (a == "--num-simulations") c.num_sims_s = need(i);
    else if (a == "--step-size") c.step_s = need(i);
    else if (a == "--fraction-to-fail") c.frac_s = need(i);
    else if (a == "--when-to-fail") u64(i, c.when_to_fail);
    else if (a == "--warm-up-rounds") u64(i, c.warm_up);
    else if (a == "--influx") c.influx = need(i);
    else if (a == "--print-stats") c.print_stats = true;
    else if (a == "--synthetic") u64(i, c.synthetic);
    else if (a == "--seed") {
      const std::string v = need(i);
      char* end = nullptr;
      c.seed = std::strtoull(v.c_str(), &end, 0);
      if (!end || *end) die(2, "invalid value '" + v + "' for --seed");
    } else if (a == "--gpus") u64(i, c.gpus);
    else if (a == "--bfs-mode") u64(i, c.bfs_mode);
    else if (a == "--save-results") c.save_results = need(i);
    else if (a == "--replay-results") c.replay_results = need(i);
    else if (a == "--engine-plan") c.engine_plan = need(i);
    else if (a == "--cluster-load") c.cluster_load = need(i);
    else if (a == "--cluster-load-by-config") c.cluster_by_config = need(i);
    else if (a == "--influx-file") c.influx_file = need(i);
    else if (a == "--influx-time-base") u64(i, c.influx_time_base);
    else if (a == "--batch-sweeps") c.batch_sweeps = true;
    else if (a == "--trials") u64(i, c.trials);
    else die(2, "unexpected argument '" + a + "' (see --help)");
  }
  return c;
}

// Accounts -> (keys, stakes) in id order (make_gossip_cluster gossip.rs:883-925).
void load_nodes(const Cli& c, std::vector<std::string>& keys, std::vector<uint64_t>& stakes) {
  std::vector<gsio::Account> acc;
  std::string err;
  if (c.accounts_from_yaml) {
    if (c.account_file.empty()) {
      gsrep::log_warn(stderr, TMAIN,
                      "Failed to pass in account file to read from with --accounts-from-yaml flag. need --acount-file <path>");
      std::exit(255);
    }
    gsrep::log_info(stderr, TMAIN, "Reading " + c.account_file);
    if (!gsio::read_stake_yaml(c.account_file, acc, err)) die(1, err);
    gsrep::log_info(stderr, TMAIN, std::to_string(acc.size()) + " accounts read in");
  } else if (c.synthetic) {
    acc = gsio::synthetic_network((uint32_t)c.synthetic);
  } else {
    die(1, "the RPC account pull (" + c.url + ") is not available offline: use --accounts-from-yaml "
           "--account-file PATH or --synthetic N");
  }
  std::vector<gsio::Account> kept;
  for (auto& a : acc) {
    if (c.filter_zero && a.stake == 0) continue;
    uint8_t pk[32];
    std::string why;
    if (!gsio::b58decode_pubkey(a.key, pk, &why)) die(1, "invalid pubkey '" + a.key + "': " + why);
    kept.push_back(a);
  }
  stakes = gsio::to_id_order(kept);
  keys.clear();
  for (auto& a : kept) keys.push_back(a.key);
}

struct Job {
  gs_sim_config cfg;
  int device = 0;
  std::vector<size_t> sims;  // global simulation indices
  std::vector<uint32_t> ranks, mi;
  std::vector<double> thr, frac;
  std::vector<uint32_t> fanouts;  // per simulation
  bool slot_fanouts = false;      // a push-fanout sweep: the engine takes `fanouts` per slot
  bool traj = false;              // --batch-sweeps: an active-set table per (size, probability) of `aszs` / `probs`
  std::vector<uint32_t> aszs;     // per simulation
  std::vector<double> probs;
  std::vector<uint64_t> seeds;    // --trials K > 1: per simulation (a table per size, probability and seed), else empty
};

void run_job(const Job& j, const std::vector<uint64_t>& stakes, std::vector<gsrep::SimArrays>& out,
             std::string& err, int cluster /*0 no view, 1 over the engine, 2 per trajectory table*/) {
  gs_sim_config cfg = j.cfg;
  cfg.device = j.device;
  gs_sim_result* r = nullptr;
  const int rc =
      cluster == 2
          ? gs_run_simulations_cluster_tables(&cfg, stakes.data(), (uint32_t)stakes.size(), (uint32_t)j.sims.size(),
                                              j.ranks.data(), j.mi.data(), j.thr.data(), j.frac.data(),
                                              j.slot_fanouts || j.traj ? j.fanouts.data() : nullptr,
                                              j.traj ? j.aszs.data() : nullptr, j.traj ? j.probs.data() : nullptr,
                                              j.traj && !j.seeds.empty() ? j.seeds.data() : nullptr, nullptr, &r)
      : cluster ? gs_run_simulations_cluster(&cfg, stakes.data(), (uint32_t)stakes.size(), (uint32_t)j.sims.size(),
                                           j.ranks.data(), j.mi.data(), j.thr.data(), j.frac.data(),
                                           j.slot_fanouts || j.traj ? j.fanouts.data() : nullptr,
                                           j.traj ? j.aszs.data() : nullptr, j.traj ? j.probs.data() : nullptr,
                                           j.traj && !j.seeds.empty() ? j.seeds.data() : nullptr, 1, &r)
      : j.traj && !j.seeds.empty()
          ? gs_run_simulations_seeds(&cfg, stakes.data(), (uint32_t)stakes.size(), (uint32_t)j.sims.size(),
                                     j.ranks.data(), j.mi.data(), j.thr.data(), j.frac.data(), j.fanouts.data(),
                                     j.aszs.data(), j.probs.data(), j.seeds.data(), &r)
      : j.traj ? gs_run_simulations_traj(&cfg, stakes.data(), (uint32_t)stakes.size(), (uint32_t)j.sims.size(),
                                       j.ranks.data(), j.mi.data(), j.thr.data(), j.frac.data(), j.fanouts.data(),
                                       j.aszs.data(), j.probs.data(), &r)
             : gs_run_simulations_fanouts(&cfg, stakes.data(), (uint32_t)stakes.size(), (uint32_t)j.sims.size(),
                                          j.ranks.data(), j.mi.data(), j.thr.data(), j.frac.data(),
                                          j.slot_fanouts ? j.fanouts.data() : nullptr, &r);
  if (rc) {
    err = std::string("gs_run_simulations: ") + gs_last_error();
    return;
  }
  // (per table: the engine's tables stand in the order of their first simulation, gs_traj_plan.h)
  std::vector<std::tuple<uint32_t, double, uint64_t>> tabs;
  for (size_t k = 0; k < j.sims.size(); ++k) {
    gsrep::SimArrays& a = out[j.sims[k]];
    bool first_of_table = false;
    if (cluster == 2) {
      const auto key = j.traj ? std::make_tuple(j.aszs[k], j.probs[k], j.seeds.empty() ? (uint64_t)0 : j.seeds[k])
                              : std::make_tuple((uint32_t)0, 0.0, (uint64_t)0);
      first_of_table = std::find(tabs.begin(), tabs.end(), key) == tabs.end();
      if (first_of_table) {
        a.u[CLUSTER_TABLE] = {(uint64_t)tabs.size()};
        tabs.push_back(key);
      }
    }
    for (const char* nm : F64_NAMES) {
      const size_t n = gs_result_f64(r, (uint32_t)k, nm, nullptr, 0);
      if (n == SIZE_MAX) continue;
      a.f[nm].resize(n);
      gs_result_f64(r, (uint32_t)k, nm, a.f[nm].data(), n);
    }
    for (const char* nm : U64_NAMES) {
      const size_t n = gs_result_u64(r, (uint32_t)k, nm, nullptr, 0);
      if (n == SIZE_MAX) continue;
      a.u[nm].resize(n);
      gs_result_u64(r, (uint32_t)k, nm, a.u[nm].data(), n);
    }
    // the engine's totals once, under its first simulation; per table: the table's, under its first
    if (cluster == 2 ? first_of_table : cluster && k == 0)
      for (const char* nm : CLUSTER_NAMES) {
        const size_t n = gs_result_u64(r, (uint32_t)k, nm, nullptr, 0);
        if (n == SIZE_MAX) continue;
        a.u[nm].resize(n);
        gs_result_u64(r, (uint32_t)k, nm, a.u[nm].data(), n);
      }
  }
  gs_result_free(r);
}

int write_accounts_main(int argc, char** argv) {
  // write_accounts_main.rs:62-127 over the synthetic network (no RPC offline)
  std::string file;
  uint64_t num_nodes = UINT64_MAX, synthetic = 0;
  bool zero_only = false, filter_zero = false;
  for (int i = 2; i < argc; ++i) {
    const std::string a = argv[i];
    auto need = [&]() -> std::string {
      if (i + 1 >= argc) die(2, "missing value for " + a);
      return argv[++i];
    };
    if (a == "--account-file") file = need();
    else if (a == "--num-nodes") { if (!parse_u64(need(), num_nodes)) die(2, "invalid --num-nodes"); }
    else if (a == "--synthetic") { if (!parse_u64(need(), synthetic)) die(2, "invalid --synthetic"); }
    else if (a == "--zero-stakes") zero_only = true;
    else if (a == "-f" || a == "--filter-zero-staked-nodes") filter_zero = true;
    else if (a == "--url") need();
    else die(2, "unexpected argument '" + a + "'");
  }
  if (file.empty()) die(2, "--account-file PATH is required");
  if (!synthetic) die(1, "the RPC account pull is not available offline: pass --synthetic N");
  std::vector<gsio::Account> nodes = gsio::synthetic_network((uint32_t)synthetic), out;
  for (auto& n : nodes) {
    if (filter_zero && n.stake == 0) continue;
    if (zero_only && n.stake != 0) continue;
    out.push_back(n);
    if (out.size() > num_nodes - 1) break;
  }
  gsrep::log_info(stderr, "write_accounts", "Writing " + file);
  std::string err;
  if (!gsio::write_stake_yaml(file, out, err)) die(1, err);
  gsrep::log_info(stderr, "write_accounts", "Wrote " + std::to_string(out.size()) + " keys to file: " + file);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc > 1 && std::strcmp(argv[1], "write-accounts") == 0) return write_accounts_main(argc, argv);
  const Cli c = parse(argc, argv);
  const uint64_t start_ns = (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(  // gossip_main.rs:724
                                std::chrono::system_clock::now().time_since_epoch()).count();

  // validators and value parsing of gossip_main.rs:120-148,248-252,655-704
  double p0 = 0, thr0 = 0, frac0 = 0;
  if (!parse_f64(c.p_s, p0) || !(p0 >= 0.0 && p0 <= 1.0))
    die(2, "active_set_rotation_probability must be between 0 and 1");
  if (!parse_f64(c.thr_s, thr0) || !(thr0 >= 0.0 && thr0 <= 1.0))
    die(2, "prune_stake_threshold must be between 0 and 1");
  if (!parse_f64(c.frac_s, frac0)) die(2, "invalid value '" + c.frac_s + "' for --fraction-to-fail");
  int test_type = gsrep::NO_TEST;
  if (!c.test_type_s.empty()) {
    test_type = gsrep::parse_test_type(c.test_type_s);
    if (test_type < 0) die(2, "Invalid test type");
  }
  uint64_t num_sims = 0;
  if (!parse_u64(c.num_sims_s, num_sims)) die(1, "Invalid num_simulations value");
  gsrep::StepSize step;
  if (!parse_u64(c.step_s, step.i)) {
    step.is_int = false;
    if (!parse_f64(c.step_s, step.f)) die(1, "Invalid step_size value");
  }
  if (c.influx != "n") die(1, "influx reporting over HTTP is not available offline (--influx n)");
  if (c.gpus < 1) die(2, "--gpus must be >= 1");
  if (c.trials < 1) die(2, "--trials must be >= 1");
  const uint64_t K = c.trials;

  if (c.origin_ranks.size() < num_sims) {
    gsrep::log_warn(stderr, TMAIN, "ERROR: not enough origin ranks provided for num_simulations! origin_ranks.len(): " +
                                       std::to_string(c.origin_ranks.size()) + ", num_simulations: " +
                                       std::to_string(num_sims));
    return 0;
  } else if (c.origin_ranks.size() > num_sims) {
    gsrep::log_warn(stderr, TMAIN, "WARNING: more origin ranks than number of simulations. Not going to hit all origin ranks");
  } else if (c.origin_ranks.size() > 1 && test_type != gsrep::ORIGIN_RANK) {
    gsrep::log_warn(stderr, TMAIN, "ERROR: multiple origin_ranks passed in but test type is not OriginRank. "
                                   "This would end up running all simulations with origin_rank[0]: " +
                                       std::to_string(c.origin_ranks[0]));
    return 0;
  }
  if (c.iterations <= c.warm_up)
    gsrep::log_warn(stderr, TMAIN, "WARNING: Gossip Iterations (" + std::to_string(c.iterations) + ") <= Warm Up Rounds (" +
                                       std::to_string(c.warm_up) + "). No stats will be recorded....");

  std::vector<std::string> keys;
  std::vector<uint64_t> stakes;
  load_nodes(c, keys, stakes);
  gsrep::log_info(stderr, "gossip_sim::gossip", "num of cluster nodes: " + std::to_string(stakes.size()));

  // per-simulation parameters (the test-type loops of gossip_main.rs:774-951)
  std::vector<gsrep::SimParams> params(num_sims);
  for (uint64_t i = 0; i < num_sims; ++i) {
    gsrep::SimParams& q = params[i];
    q.gossip_push_fanout = c.fanout;
    q.gossip_active_set_size = c.asz;
    q.gossip_iterations = c.iterations;
    q.origin_rank = c.origin_ranks[0];
    q.probability_of_rotation = p0;
    q.prune_stake_threshold = thr0;
    q.min_ingress_nodes = c.min_ingress;
    q.fraction_to_fail = frac0;
    q.when_to_fail = c.when_to_fail;
    q.test_type = test_type;
    q.num_simulations = num_sims;
    q.step_size = step;
    switch (test_type) {
      case gsrep::ACTIVE_SET_SIZE: q.gossip_active_set_size = c.asz + i * step.as_usize(); break;
      case gsrep::PUSH_FANOUT:
        q.gossip_push_fanout = c.fanout + i * step.as_usize();
        if (q.gossip_push_fanout > q.gossip_active_set_size) q.gossip_active_set_size = q.gossip_push_fanout;
        break;
      case gsrep::MIN_INGRESS_NODES: q.min_ingress_nodes = c.min_ingress + i * step.as_usize(); break;
      case gsrep::PRUNE_STAKE_THRESHOLD: q.prune_stake_threshold = thr0 + (double)i * step.as_f64(); break;
      case gsrep::ORIGIN_RANK: q.origin_rank = c.origin_ranks[i]; break;
      case gsrep::FAIL_NODES: q.fraction_to_fail = frac0 + (double)i * step.as_f64(); break;
      case gsrep::ROTATE_PROBABILITY: q.probability_of_rotation = p0 + (double)i * step.as_f64(); break;
      default: break;
    }
    if (stakes.size() < q.origin_rank)
      die(101, "ERROR: origin_rank larger than number of simulation nodes. nodes.len(): " + std::to_string(stakes.size()) +
                   ", origin_rank: " + std::to_string(q.origin_rank));
  }

  // engines: sims sharing (active-set size, rotation probability) batch into one
  std::vector<Job> jobs;
  if (num_sims) {
    auto base_cfg = [&](const gsrep::SimParams& q) {
      gs_sim_config cfg{};
      cfg.push_fanout = (uint32_t)q.gossip_push_fanout;
      cfg.active_set_size = (uint32_t)q.gossip_active_set_size;
      cfg.iterations = (uint32_t)c.iterations;
      cfg.warm_up_rounds = (uint32_t)c.warm_up;
      cfg.min_ingress_nodes = (uint32_t)q.min_ingress_nodes;
      cfg.when_to_fail = (uint32_t)c.when_to_fail;
      cfg.rotation_probability = std::min(q.probability_of_rotation, 1.0);  // gen::<f64>() < p: p > 1 acts as 1
      cfg.prune_stake_threshold = q.prune_stake_threshold;
      cfg.fraction_to_fail = q.fraction_to_fail;
      cfg.num_buckets_stranded = c.nb_stranded;
      cfg.num_buckets_message = c.nb_message;
      cfg.num_buckets_hops = c.nb_hops;
      cfg.test_type = test_type;
      cfg.seed = c.seed;
      cfg.bfs_mode = (uint32_t)c.bfs_mode;
      return cfg;
    };
    const bool per_value_engine = test_type == gsrep::ACTIVE_SET_SIZE || test_type == gsrep::ROTATE_PROBABILITY;
    // --batch-sweeps: the sweeps whose value changes the trajectory (and a push-fanout sweep's
    // sims of raised size) as tables of one engine, when the network fits the workgroup engine
    // (--trials: the seeds are tables too, so every test type batches)
    bool traj = c.batch_sweeps && (per_value_engine || test_type == gsrep::PUSH_FANOUT || K > 1);
    if (traj) {
      uint64_t fmax = 1, amax = 1;
      for (const auto& q : params) { fmax = std::max(fmax, q.gossip_push_fanout); amax = std::max(amax, q.gossip_active_set_size); }
      if (c.bfs_mode == GS_BFS_MULTI) {  // the tables on the multi-source BFS: any node count it supports
        if (amax > GS_MAX_ACTIVE_SET_SIZE ||
            !gs_traj_multi_supported((uint32_t)stakes.size(), (uint32_t)std::min<uint64_t>(num_sims * K, 0xFFFFFFFFu),
                                     (uint32_t)std::min<uint64_t>(fmax, 0xFFFFFFFFu), (uint32_t)amax)) {
          gsrep::log_info(stderr, TMAIN, "--batch-sweeps: " + std::to_string(stakes.size()) + " nodes at active-set size " +
                                             std::to_string(amax) + " do not fit the multi-source table engine; planning one engine per value");
          traj = false;
        }
      } else if (amax > GS_MAX_ACTIVE_SET_SIZE ||
          !gs_traj_supported((uint32_t)stakes.size(), (uint32_t)std::min<uint64_t>(fmax, 0xFFFFFFFFu), (uint32_t)amax, nullptr)) {
        gsrep::log_info(stderr, TMAIN, "--batch-sweeps: " + std::to_string(stakes.size()) + " nodes at active-set size " +
                                           std::to_string(amax) + " do not fit the workgroup engine; planning one engine per value");
        traj = false;
      }
    }
    // batches: sims that share a trajectory (or, batched, an engine), in simulation order
    std::vector<std::vector<size_t>> batches;
    if (traj) {
      batches.emplace_back();
      for (size_t i = 0; i < num_sims; ++i) batches[0].push_back(i);
    } else if (per_value_engine) {
      for (size_t i = 0; i < num_sims; ++i) batches.push_back({i});
    } else if (test_type == gsrep::PUSH_FANOUT) {  // the sims of one (raised) active-set size
      for (size_t i = 0; i < num_sims; ++i) {
        size_t b = 0;
        while (b < batches.size() &&
               params[batches[b][0]].gossip_active_set_size != params[i].gossip_active_set_size)
          ++b;
        if (b == batches.size()) batches.emplace_back();
        batches[b].push_back(i);
      }
    } else {
      batches.emplace_back();
      for (size_t i = 0; i < num_sims; ++i) batches[0].push_back(i);
    }
    // a batch is split into contiguous chunks over the devices
    std::vector<std::vector<size_t>> groups;
    for (const auto& b : batches) {
      const size_t K = std::min<size_t>(c.gpus, b.size());
      for (size_t d = 0; d < K; ++d)
        groups.emplace_back(b.begin() + b.size() * d / K, b.begin() + b.size() * (d + 1) / K);
    }
    // --trials K > 1: unit i * K + k is simulation i at seed + k. Batched, the units of every
    // value are one batch (split over the devices as above); else today's plan once per seed.
    struct Unit { std::vector<size_t> sims; uint64_t k; };  // k: the trial (batched: unused)
    std::vector<Unit> units;
    if (K == 1) {
      for (const auto& g : groups) units.push_back(Unit{g, 0});
    } else if (traj) {
      const size_t U = num_sims * K, D = std::min<size_t>(c.gpus, U);
      for (size_t d = 0; d < D; ++d) {
        Unit u{{}, 0};
        for (size_t x = U * d / D; x < U * (d + 1) / D; ++x) u.sims.push_back(x);
        units.push_back(std::move(u));
      }
    } else {
      for (const auto& g : groups)
        for (uint64_t k = 0; k < K; ++k) units.push_back(Unit{g, k});
    }
    for (size_t gi = 0; gi < units.size(); ++gi) {
      Job j;
      const bool by_unit = K > 1 && traj;  // the job's sims are unit indices
      std::vector<size_t> vals;            // the simulation (value) of each of the job's sims
      for (size_t x : units[gi].sims) vals.push_back(by_unit ? x / K : x);
      j.cfg = base_cfg(params[vals[0]]);
      j.device = (int)(gi % c.gpus);
      if (K == 1) j.sims = units[gi].sims;
      else if (by_unit) { j.sims = units[gi].sims; for (size_t x : j.sims) j.seeds.push_back(c.seed + x % K); }
      else { for (size_t i : vals) j.sims.push_back(i * K + units[gi].k); j.cfg.seed = c.seed + units[gi].k; }
      j.slot_fanouts = test_type == gsrep::PUSH_FANOUT;
      j.traj = traj;
      for (size_t i : vals) {
        j.aszs.push_back((uint32_t)params[i].gossip_active_set_size);
        j.probs.push_back(std::min(params[i].probability_of_rotation, 1.0));
        j.ranks.push_back((uint32_t)params[i].origin_rank);
        j.mi.push_back((uint32_t)params[i].min_ingress_nodes);
        j.thr.push_back(params[i].prune_stake_threshold);
        j.frac.push_back(params[i].fraction_to_fail);
        j.fanouts.push_back((uint32_t)params[i].gossip_push_fanout);
      }
      if (j.slot_fanouts || j.traj) j.cfg.push_fanout = *std::max_element(j.fanouts.begin(), j.fanouts.end());
      jobs.push_back(std::move(j));
    }
  }
  if (!c.engine_plan.empty()) {  // (before any engine exists; also with --replay-results)
    FILE* f = std::fopen(c.engine_plan.c_str(), "w");
    if (!f) die(1, "cannot write " + c.engine_plan);
    for (const Job& j : jobs) {
      std::fprintf(f, "device %d sims ", j.device);
      for (size_t k = 0; k < j.sims.size(); ++k) std::fprintf(f, "%s%zu", k ? "," : "", j.sims[k]);
      if (j.traj) {  // per-simulation lists
        std::fprintf(f, " active-set-size ");
        for (size_t k = 0; k < j.aszs.size(); ++k) std::fprintf(f, "%s%u", k ? "," : "", j.aszs[k]);
        std::fprintf(f, " fanouts ");
      } else {
        std::fprintf(f, " active-set-size %u fanouts ", j.cfg.active_set_size);
      }
      for (size_t k = 0; k < j.fanouts.size(); ++k) std::fprintf(f, "%s%u", k ? "," : "", j.fanouts[k]);
      if (j.traj) {
        std::fprintf(f, " rotation-probability ");
        for (size_t k = 0; k < j.probs.size(); ++k) std::fprintf(f, "%s%.17g", k ? "," : "", j.probs[k]);
      }
      if (K > 1) {  // (only then: without --trials the lines stay as they were)
        std::fprintf(f, " seeds ");
        if (j.seeds.empty()) std::fprintf(f, "%" PRIu64, j.cfg.seed);
        for (size_t k = 0; k < j.seeds.size(); ++k) std::fprintf(f, "%s%" PRIu64, k ? "," : "", j.seeds[k]);
      }
      std::fprintf(f, "\n");
    }
    std::fclose(f);
  }

  if (K > 1) {  // every repeat is a simulation of its own from here on (value-major, trial-minor)
    std::vector<gsrep::SimParams> rep;
    for (uint64_t i = 0; i < num_sims; ++i)
      for (uint64_t k = 0; k < K; ++k) rep.push_back(params[i]);
    params = std::move(rep);
    num_sims *= K;
  }
  std::vector<gsrep::SimArrays> sims(num_sims);
  if (!c.replay_results.empty()) {
    std::string err;
    if (!gsrep::load_results(c.replay_results, sims, err)) die(1, err);
    if (sims.size() != num_sims) die(1, "results file holds " + std::to_string(sims.size()) + " simulations, not " +
                                            std::to_string(num_sims));
  } else if (num_sims) {
    for (size_t i = 0; i < num_sims; ++i)
      gsrep::log_info(stderr, TMAIN, "##### SIMULATION ITERATION: " + std::to_string(i) + " #####");
    // one worker thread per requested device; workers beyond the visible devices share
    // them (engines are independent), so the split itself runs on any box
    int ndev = 0;
    gs_device_count(&ndev);
    std::vector<std::string> errs(c.gpus);
    std::vector<std::thread> th;
    for (uint64_t d = 0; d < c.gpus; ++d)
      th.emplace_back([&, d]() {
        for (auto& j : jobs) {
          if ((uint64_t)j.device != d || !errs[d].empty()) continue;
          Job jj = j;
          jj.device = ndev > 0 ? (int)(d % (uint64_t)ndev) : 0;
          run_job(jj, stakes, sims, errs[d], !c.cluster_by_config.empty() ? 2 : !c.cluster_load.empty() ? 1 : 0);
        }
      });
    for (auto& t : th) t.join();
    for (auto& e : errs)
      if (!e.empty()) die(1, e);
    for (size_t i = 0; i < num_sims; ++i) {
      const auto& o = sims[i].u["origin"];
      if (!o.empty()) gsrep::log_info(stderr, TMAIN, "ORIGIN: " + keys[o[0]]);
    }
  }
  if (!c.save_results.empty()) {
    std::string err;
    if (!gsrep::save_results(c.save_results, sims, err)) die(1, err);
  }
  if (!c.cluster_load.empty()) {  // totals are additive: summed over every engine's (over --gpus workers too)
    const size_t nn = stakes.size();
    std::vector<std::vector<uint64_t>> tot(5, std::vector<uint64_t>(nn, 0));
    bool any = false;
    for (const auto& sm : sims)
      for (size_t w = 0; w < 5; ++w) {
        const auto it = sm.u.find(CLUSTER_NAMES[w]);
        if (it == sm.u.end()) continue;
        if (it->second.size() != nn)
          die(1, std::string(CLUSTER_NAMES[w]) + " holds " + std::to_string(it->second.size()) + " nodes, not " +
                     std::to_string(nn));
        any = true;
        for (size_t v = 0; v < nn; ++v) tot[w][v] += it->second[v];
      }
    if (!any && num_sims && !c.replay_results.empty())
      die(1, c.replay_results + " holds no cluster_* totals (it was saved without --cluster-load)");
    FILE* f = std::fopen(c.cluster_load.c_str(), "w");
    if (!f) die(1, "cannot write " + c.cluster_load);
    for (size_t v = 0; v < nn; ++v)
      std::fprintf(f, "%s,%" PRIu64 ",%" PRIu64 ",%" PRIu64 ",%" PRIu64 ",%" PRIu64 ",%" PRIu64 "\n", keys[v].c_str(),
                   stakes[v], tot[0][v], tot[1][v], tot[2][v], tot[3][v], tot[4][v]);
    std::fclose(f);
  }
  if (!c.cluster_by_config.empty()) {  // one block of lines per (engine of the plan, table), in plan order
    const size_t nn = stakes.size();
    bool any = false;
    for (const Job& j : jobs)
      for (size_t i : j.sims) any = any || (i < sims.size() && sims[i].u.count(CLUSTER_TABLE));
    if (!any && num_sims && !c.replay_results.empty())
      die(1, c.replay_results + " holds no cluster_table totals (it was saved without --cluster-load-by-config)");
    struct Block { size_t engine; uint64_t table; const std::vector<uint64_t>* tot[5]; };
    std::vector<Block> blocks;  // (checked before the file is created)
    for (size_t e = 0; e < jobs.size(); ++e)
      for (size_t i : jobs[e].sims) {
        if (i >= sims.size()) continue;
        const auto tt = sims[i].u.find(CLUSTER_TABLE);
        if (tt == sims[i].u.end() || tt->second.empty()) continue;
        Block b{e, tt->second[0], {}};
        for (size_t w = 0; w < 5; ++w) {
          const auto it = sims[i].u.find(CLUSTER_NAMES[w]);
          if (it == sims[i].u.end() || it->second.size() != nn)
            die(1, std::string(CLUSTER_NAMES[w]) + " of simulation " + std::to_string(i) + " does not hold " +
                       std::to_string(nn) + " nodes");
          b.tot[w] = &it->second;
        }
        blocks.push_back(b);
      }
    FILE* f = std::fopen(c.cluster_by_config.c_str(), "w");
    if (!f) die(1, "cannot write " + c.cluster_by_config);
    for (const Block& b : blocks)
      for (size_t v = 0; v < nn; ++v)
        std::fprintf(f, "%zu,%" PRIu64 ",%s,%" PRIu64 ",%" PRIu64 ",%" PRIu64 ",%" PRIu64 ",%" PRIu64 ",%" PRIu64 "\n",
                     b.engine, b.table, keys[v].c_str(), stakes[v], (*b.tot[0])[v], (*b.tot[1])[v], (*b.tot[2])[v],
                     (*b.tot[3])[v], (*b.tot[4])[v]);
    std::fclose(f);
  }
  if (!c.influx_file.empty()) {  // the datapoint queue's text, in enqueue order (gossip_main.rs:372-645)
    gsrep::ReportInput in;
    in.keys = keys;
    in.stakes = stakes;
    in.iterations = c.iterations;
    in.warm_up_rounds = c.warm_up;
    in.num_simulations = num_sims;
    in.test_type = test_type;
    in.nb_stranded = c.nb_stranded;
    in.nb_message = c.nb_message;
    in.nb_hops = c.nb_hops;
    in.params = params;
    in.sims = sims;
    gsrep::InfluxOptions io;
    io.time_base = c.influx_time_base;
    io.start_time = std::to_string(c.influx_time_base ? c.influx_time_base : start_ns);
    io.api = c.accounts_from_yaml ? c.account_file : "synthetic:" + std::to_string(c.synthetic);
    if (num_sims) {
      const gsrep::SimParams& q = params[0];
      switch (test_type) {
        case gsrep::ACTIVE_SET_SIZE: io.start_value = (double)q.gossip_active_set_size; break;
        case gsrep::PUSH_FANOUT: io.start_value = (double)c.fanout; break;
        case gsrep::MIN_INGRESS_NODES: io.start_value = (double)q.min_ingress_nodes; break;
        case gsrep::PRUNE_STAKE_THRESHOLD: io.start_value = q.prune_stake_threshold; break;
        case gsrep::ORIGIN_RANK: io.start_value = (double)q.origin_rank; break;
        case gsrep::FAIL_NODES: io.start_value = q.fraction_to_fail; break;
        case gsrep::ROTATE_PROBABILITY: io.start_value = q.probability_of_rotation; break;
        default: break;
      }
    }
    FILE* f = std::fopen(c.influx_file.c_str(), "w");
    if (!f) die(1, "cannot write " + c.influx_file);
    gsrep::write_influx(f, in, io);
    std::fclose(f);
  }
  if (c.print_stats) {
    // GossipStatsCollection holds only simulations that recorded rounds (gossip_main.rs:567-593)
    gsrep::ReportInput in;
    in.keys = keys;
    in.stakes = stakes;
    in.iterations = c.iterations;
    in.warm_up_rounds = c.warm_up;
    in.num_simulations = num_sims;
    in.test_type = test_type;
    in.nb_stranded = c.nb_stranded;
    in.nb_message = c.nb_message;
    in.nb_hops = c.nb_hops;
    if (c.iterations > c.warm_up) {
      in.params = params;
      in.sims = sims;
    }
    if (!in.sims.empty()) gsrep::print_all(stderr, in);
    else gsrep::log_warn(stderr, TMAIN, "WARNING: Gossip Stats Collection is empty. Is `Iterations` <= `warm-up-rounds`?");
  }
  return 0;
}
