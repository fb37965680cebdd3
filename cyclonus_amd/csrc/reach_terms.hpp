// reach_terms.hpp — the host arithmetic of cyc_table_reach (reach.hpp) that is not a launch: the checks of the seed
// lists and of the working set, the seed lists as the initial bitsets of the search, and `levels` from the counters a
// step delivers (dev_reach.hpp).  Plain integer C++ without HIP (tests/native/reach_terms_check.cpp runs it on the CPU).
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "cyclonus_hip.h"

namespace cyc {

// seed sets x 64-pod words of one call: three bitsets of that many words and 64 times as many 32-bit hop values
// live on the device during the call (include/cyclonus_hip.h states the limit)
constexpr int64_t REACH_WORDS_MAX = int64_t(1) << 24;

// The checks of the seed lists; nullptr when they are fine (`why` holds a built message).  Nothing behind this
// indexes by a seed that it has not seen: it is the guard of the bitsets and of the device's row gather.
inline const char* reach_seeds_bad(int64_t P, const int64_t* seed_off, const int32_t* seeds, int64_t n_sets, std::string& why) {
  if (n_sets < 0) return "negative n_sets";
  if (!seed_off) return "null seed_off";
  if (seed_off[0] != 0) return "seed_off must start at 0 and never decrease";
  for (int64_t j = 0; j < n_sets; j++)
    if (seed_off[j + 1] < seed_off[j]) return "seed_off must start at 0 and never decrease";
  const int64_t n = seed_off[n_sets];
  if (n > 0 && !seeds) return "null seeds";
  for (int64_t i = 0; i < n; i++)
    if (seeds[i] < 0 || seeds[i] >= P) {
      why = "seeds[" + std::to_string(i) + "] = " + std::to_string(seeds[i]) + " is not a pod in [0, " + std::to_string(P) + ")";
      return why.c_str();
    }
  return nullptr;
}

// words of one bitset over all the sets, or the refusal
inline const char* reach_size_bad(int64_t W, int64_t n_sets) {
  const int64_t w = W > 0 ? W : 1;
  return n_sets > REACH_WORDS_MAX / w ? "n_sets * words exceeds the limit of 16777216 (2^24)" : nullptr;
}

// The seed lists (checked) as bitsets [n_sets][W]: bit p of set j's words = p is a seed of set j.  levels [n_sets]:
// 0 for a set with a seed (its seeds are at hop 0), -1 for an empty set.
inline void reach_seed_bits(int64_t W, const int64_t* seed_off, const int32_t* seeds, int64_t n_sets, std::vector<uint64_t>& bits,
                            std::vector<int64_t>& levels) {
  bits.assign(size_t(n_sets * W), 0);
  levels.assign(size_t(n_sets), -1);
  for (int64_t j = 0; j < n_sets; j++)
    for (int64_t i = seed_off[j]; i < seed_off[j + 1]; i++) {
      const int64_t p = seeds[i];
      bits[size_t(j * W + p / 64)] |= uint64_t(1) << (p % 64);
      levels[size_t(j)] = 0;
    }
}

// After the step of hop `hop`: cnt[j] = pods of set j first reached at that hop.  Such a set's level is now `hop`;
// returns whether any set found a pod (otherwise the search is at its fixpoint).
inline bool reach_levels(const unsigned long long* cnt, int64_t n_sets, int64_t hop, int64_t* levels) {
  bool any = false;
  for (int64_t j = 0; j < n_sets; j++)
    if (cnt[j]) levels[j] = hop, any = true;
  return any;
}

}  // namespace cyc
