#!/usr/bin/env python3
"""Busy span and round-to-round gaps of k_round_wg from a rocprofv3 --kernel-trace CSV.

With the round split (GS_ROUND_SPLIT) a round is two launches on two streams, so a launch
average says little; what the split is for shows in two figures over a window of rounds:
  busy_us      time in which at least one k_round_wg launch runs (the union of the intervals)
  gap_us       per round, from the end of the round's last launch to the start of the next
               round's first launch (negative: the next round began while this one still ran)
and, with two launches per round, in how many rounds the next round's first launch started
before this round's last one ended.

  python3 scripts/round_gap.py --csv .../run_kernel_trace.csv --per-round 2 --first 20 --count 100
"""
import argparse
import csv
import json


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--csv", required=True)
    ap.add_argument("--kernel", default="k_round_wg")
    ap.add_argument("--per-round", type=int, default=1, help="launches per round (2 with the split on)")
    ap.add_argument("--first", type=int, default=20, help="first round of the window")
    ap.add_argument("--count", type=int, default=100)
    a = ap.parse_args()
    rows = []
    with open(a.csv) as f:
        for r in csv.DictReader(f):
            if a.kernel in r["Kernel_Name"]:
                rows.append((int(r["Dispatch_Id"]), int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    rows.sort()
    n = a.per_round
    rounds = [rows[i * n:(i + 1) * n] for i in range(len(rows) // n)]
    win = rounds[a.first:a.first + a.count]
    if len(win) != a.count:
        raise SystemExit(f"{len(rounds)} rounds of {a.kernel}; window [{a.first}, {a.first + a.count}) incomplete")
    iv = sorted((s, e) for rd in win for _, s, e in rd)
    busy, cs, ce = 0, iv[0][0], iv[0][1]
    for s, e in iv[1:]:
        if s > ce:
            busy += ce - cs
            cs, ce = s, e
        else:
            ce = max(ce, e)
    busy += ce - cs
    gaps, early = [], 0
    nxt = rounds[a.first + 1:a.first + a.count + 1]
    for rd, nx in zip(win, nxt):
        g = min(s for _, s, _ in nx) - max(e for _, _, e in rd)
        gaps.append(g / 1e3)
        early += g < 0
    span = max(e for _, e in iv) - min(s for s, _ in iv)
    out = {"rounds": [a.first, a.first + a.count], "launches_per_round": n,
           "span_us_per_round": span / 1e3 / a.count, "busy_us_per_round": busy / 1e3 / a.count,
           "sum_of_launches_us_per_round": sum(e - s for s, e in iv) / 1e3 / a.count,
           "gap_us_avg": sum(gaps) / len(gaps), "gap_us_min": min(gaps), "gap_us_max": max(gaps),
           "rounds_started_before_the_last_ended": early, "gaps_counted": len(gaps)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
