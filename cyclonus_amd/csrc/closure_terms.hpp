// closure_terms.hpp — the host arithmetic of cyc_table_closure and cyc_table_zones (closure.hpp) that is not a launch:
// the argument messages, the check of the representatives k_closure_zones delivers (dev_closure.hpp) and the canonical
// zone numbering from them.  Plain integer C++ without HIP (tests/native/closure_terms_check.cpp runs it on the CPU).
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "cyclonus_hip.h"

namespace cyc {

// words of a row of the closure's scratch plane: W rounded up to whole 128-byte lines
inline uint64_t closure_pitch(uint64_t W) { return (W + 15) / 16 * 16; }

// cyc_table_closure's outputs; nullptr when they are fine
inline const char* closure_outputs_bad(const void* d_closure, const void* n_reach) {
  if (reinterpret_cast<uintptr_t>(d_closure) % 8) return "d_closure is not 8-byte aligned";
  if (!d_closure && !n_reach) return "no output requested";
  return nullptr;
}

// cyc_table_zones' outputs
inline const char* zones_outputs_bad(const void* zone, const void* n_zones, const void* n_from, const void* n_to) {
  return !zone && !n_zones && !n_from && !n_to ? "no output requested" : nullptr;
}

// rep[p]: the smallest pod q such that p reaches q and q reaches p.  Mutual reachability is an equivalence, so every
// pod's representative is at most the pod and is its own representative; anything else means the closure plane was not
// a closure.  nullptr when they are fine (`why` holds a built message).
inline const char* zone_reps_bad(const uint32_t* rep, int64_t P, std::string& why) {
  for (int64_t p = 0; p < P; p++) {
    const int64_t q = rep[p];
    if (q > p || int64_t(rep[q]) != q) {
      why = "internal: rep[" + std::to_string(p) + "] = " + std::to_string(q) + " is not the smallest pod of a zone";
      return why.c_str();
    }
  }
  return nullptr;
}

// Zones numbered 0, 1, ... in the order of their smallest member pod (cyc_table_classes' convention): the id of a zone
// is the rank of its representative.  rep as checked by zone_reps_bad; zone may be null.  Returns the number of zones.
inline int64_t zone_number(const uint32_t* rep, int64_t P, int32_t* zone, std::vector<int32_t>& id) {
  id.assign(size_t(P), 0);
  int32_t n = 0;
  for (int64_t p = 0; p < P; p++) {
    id[size_t(p)] = int64_t(rep[p]) == p ? n++ : id[rep[p]];  // (rep[p] < p: numbered already)
    if (zone) zone[p] = id[size_t(p)];
  }
  return n;
}

}  // namespace cyc
