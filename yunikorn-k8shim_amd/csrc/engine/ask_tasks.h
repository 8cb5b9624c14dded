// What every per-ask query of the engine (ykpred_explain, ykpred_headroom*, ykpred_preempt_*: include/ykpred.h) does on the host around
// its kernel, plain C++ with no device header: it runs in engine.hip on every rank alike, and in tests/c/ask_tasks.cpp without a device.
//
//   partition        a list of asks → its TASKS, the distinct rows the kernel evaluates; ask i reads row task_of[i]
//   agreement_words  the two words the ranks of a node-sharded engine compare before anybody enters a reduce
//   best_key_fixup   the packed best key of ykpred_preempt_reach and ykpred_preempt_victims → [level, node, pods] of one row
#pragma once
#include <cstdint>
#include <unordered_map>
#include <vector>

namespace yktasks {
constexpr int32_t kNoNodeName = -1;  // (YKPRED_NO_NODE_NAME)

struct Partition {
  std::vector<int32_t> task_of, spec, pin;  // ask i of the list → its task; per task the spec and the NodeName pin
  std::vector<int32_t> extra_of;            // per task the extra value (empty without one)
};

// Tasks are the distinct (spec, pin) of the list, numbered by first appearance. `extra` ([n_asks] or null) is a small per-ask value
// (0..15, ykpred_preempt_reach: the limit) that is part of the key: bits 59..62, free under 2^27 specs and above an ask index. A sharded
// engine cannot key on the pin (a node index of ITS shard): an ask with a NodeName is a task of its own there, and with by_ask every
// distinct ask index is — the keys every rank derives alike whatever its own spec table merges.
inline void partition(const int32_t* pod_spec, const int32_t* pod_pin, int32_t n_asks, const int32_t* asks, const int32_t* extra, bool sharded,
                      bool by_ask, Partition* out) {
  std::unordered_map<uint64_t, int32_t> index;
  out->task_of.assign((size_t)(n_asks > 0 ? n_asks : 0), 0);
  out->spec.clear();
  out->pin.clear();
  out->extra_of.clear();
  for (int i = 0; i < n_asks; ++i) {
    const int32_t a = asks[i], sp = pod_spec[(size_t)a], pin = pod_pin[(size_t)a];
    uint64_t key = ((uint64_t)(uint32_t)sp << 32) | (uint64_t)(uint32_t)pin;
    if (by_ask || (sharded && pin != kNoNodeName)) key = (1ull << 63) | (uint64_t)(uint32_t)a;
    if (extra) key |= (uint64_t)(extra[i] & 15) << 59;
    auto it = index.emplace(key, (int32_t)out->spec.size());
    if (it.second) {
      out->spec.push_back(sp);
      out->pin.push_back(pin);
      if (extra) out->extra_of.push_back(extra[i]);
    }
    out->task_of[(size_t)i] = it.first->second;
  }
}

// FNV-1a over the ask indices and over their task numbers. Ranks whose lists differ fail the call; ranks whose partitions differ (per-shard
// dictionaries merge specs differently) all fall back to by_ask.
constexpr uint64_t kHashSeed = 0x9e3779b97f4a7c15ull, kHashPrime = 0x100000001b3ull;
inline void agreement_words(int32_t n_asks, const int32_t* asks, const int32_t* task_of, uint64_t* list, uint64_t* part) {
  *list = *part = kHashSeed;
  for (int i = 0; i < n_asks; ++i) {
    *list = (*list ^ (uint64_t)(uint32_t)asks[i]) * kHashPrime;
    *part = (*part ^ (uint64_t)(uint32_t)task_of[(size_t)i]) * kHashPrime;
  }
}

// A best key packs (level << 59) | (min(pods, kBestPodsMax) << 31) | node, so the MIN over nodes and shards is the lowest level, then the
// fewest pods, then the lowest node; the column is seeded with 0x7f bytes (level field 15: no node).
constexpr int kBestLevelShift = 59, kBestPodsShift = 31, kBestMaxLevel = 8;
constexpr int64_t kBestPodsMax = (1ll << 28) - 1;

// One reduced row of `cells` cells with five consecutive ones at `at`: [at] status (arrives as the number of shards whose spec table
// does not evaluate the spec), [at + 1] limit, [at + 2] level, [at + 3] node, [at + 4] pods of the best node.
inline void best_key_fixup(int64_t* row, int cells, int at, uint64_t key, int64_t limit) {
  const int64_t level = (int64_t)(key >> kBestLevelShift);
  if (row[at] != 0) {
    for (int c = 0; c < cells; ++c) row[c] = 0;
    row[at] = 1;
    row[at + 3] = -1;
  } else if (level >= 1 && level <= kBestMaxLevel) {
    row[at + 2] = level;
    row[at + 3] = (int64_t)(key & 0x7fffffffull);
    row[at + 4] = (int64_t)((key >> kBestPodsShift) & (uint64_t)kBestPodsMax);
  } else {
    row[at + 3] = -1;
  }
  row[at + 1] = limit;
}
}  // namespace yktasks
