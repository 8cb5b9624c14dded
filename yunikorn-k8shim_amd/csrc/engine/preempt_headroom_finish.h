// The finish step of ykpred_preempt_headroom (include/ykpred.h), plain C++ with no device header: it runs on the host after the reduce,
// on every rank alike, and in tests/c/preempt_headroom_finish.cpp without a device.
//
// k_preempt_headroom leaves PER-LEVEL DELTAS in a [tasks][32] table: [0..8] the copies that level L adds over level L - 1 (level 0: the
// copies of the cluster as it stands), [9..17] the nodes whose first copy arrives at level L, [18..26] the pods of the tiers that the
// nodes rising at level L had not paid for yet, [27] how many shards do not evaluate the spec. preempt_headroom_finish turns one such
// row into the 32 cells of one ask.
#pragma once
#include <cstdint>

namespace ykfinish {
constexpr int kPreemptHeadroomCells = 32;
constexpr int kPreemptHeadroomLevels = 9;  // levels 0 .. 8

// deltas[32] → out[32] (may not alias). limit 0 .. 8, want >= 1: the caller checked both. The deltas above the limit are zero (the
// kernel's walk ends at the limit), so the prefix sums are flat there.
inline void preempt_headroom_finish(const int64_t* deltas, int64_t limit, int64_t want, bool coupled, int64_t* out) {
  for (int c = 0; c < kPreemptHeadroomCells; ++c) out[c] = 0;
  out[28] = limit;
  out[29] = want;
  if (deltas[27] != 0) {  // routed: the spec is YKPRED_SPEC_UNSUPPORTED
    out[27] = 1;
    return;
  }
  for (int row = 0; row < 3; ++row) {
    int64_t sum = 0;
    for (int l = 0; l < kPreemptHeadroomLevels; ++l) {
      sum += deltas[row * kPreemptHeadroomLevels + l];
      out[row * kPreemptHeadroomLevels + l] = sum;
    }
  }
  out[30] = -1;
  if (coupled) {  // copies change each other's verdicts: only the single-copy fit counts stand
    for (int l = 0; l < kPreemptHeadroomLevels; ++l) out[l] = out[18 + l] = -1;
    out[27] = 2;
    return;
  }
  for (int l = 0; l < kPreemptHeadroomLevels && l <= limit; ++l)
    if (out[l] >= want) {
      out[30] = l;
      break;
    }
}
}  // namespace ykfinish
