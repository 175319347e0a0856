// gs_split_plan.h -- generations of the round split (plain C++, no device code: gs_engine.hip
// drives the split rounds with it and tests/split_plan_check.cpp checks it stand-alone).
//
// With the round split on, the slots run as two groups on two streams and the groups may be one
// round apart: group 1's round k starts once group 0's round k - 1 has ended, and group 0's round
// k once group 1's round k - 2 has ended. Rotation k runs inside group 0's round k. So while
// rotation k writes, rounds k - 1 and k may still read: rows and rotation lists (nodes, changed
// bits, counter) each have three generations.
//
//   rows:  round k reads generation `read`; rotation k writes `write`, the generation that round
//          k - 2 read (or any other one right after a reset, when all three are equal). Before it
//          rotates, it copies the entries of the rotations named by `catch1` (k - 1) and `catch2`
//          (k - 2) from `read` into `write`: `write` last held the rows of round k - 2, so exactly
//          these two rotations separate it from `read`.
//   lists: rotation k writes list generation `list`, the one neither k - 1 nor k - 2 wrote
//          (rotation k - 3's, last read by round k - 2's pending clear and by rotation k - 1's
//          catch-up). Round k's slots clear the prune bits named by `catch1` (the last rotation).
//
// A reset (the rows changed in place, or the first split round) makes the three row generations
// equal by whole copies and forgets the lists; a join (the primary stream waits for the other)
// changes nothing here.
#pragma once
#include <stdint.h>

namespace gs {

struct SplitStep {
  int read;    // row generation the round's slots (and the catch-up copy) read
  int write;   // row generation the round's rotation writes (the next round reads it)
  int list;    // list generation the round's rotation writes
  int catch1;  // list generation of the last rotation (-1: none since the reset)
  int catch2;  // list generation of the rotation before it (-1: none)
  // rounds (counted since the reset) whose end the groups' launches wait for (-1: none)
  int64_t g0_waits_g1;  // group 0's launch: group 1's round k - 2
  int64_t g1_waits_g0;  // group 1's launch: group 0's round k - 1
};

struct SplitPlan {
  int64_t k = 0;          // rounds since the reset
  int cur = 0;            // generation the next round reads
  int prev = -1;          // generation the last round read
  int p1 = -1, p2 = -1;   // list generations of the last two rotations

  // all three row generations now equal generation `cur_gen`; no rotation list is valid
  void reset(int cur_gen) { k = 0; cur = cur_gen; prev = -1; p1 = p2 = -1; }

  static int third(int a, int b) {  // a generation that is neither a nor b (either may be -1)
    for (int g = 0; g < 3; ++g)
      if (g != a && g != b) return g;
    return 0;
  }

  SplitStep next() {
    SplitStep s;
    s.read = cur;
    s.write = third(cur, prev);
    s.list = third(p1, p2);
    s.catch1 = p1;
    s.catch2 = p2;
    s.g0_waits_g1 = k >= 2 ? k - 2 : -1;
    s.g1_waits_g0 = k >= 1 ? k - 1 : -1;
    prev = cur;
    cur = s.write;
    p2 = p1;
    p1 = s.list;
    ++k;
    return s;
  }
};

}  // namespace gs
