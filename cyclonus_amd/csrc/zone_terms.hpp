// zone_terms.hpp — the host arithmetic of cyc_table_zone_graph (zone_graph.hpp) that is not a launch: the argument and
// capacity messages, the zones' smallest pods and sizes, the check of the edge list the device delivers and the tiers
// by a topological pass over it.  Plain integer C++ without HIP (tests/native/zone_terms_check.cpp runs it on the CPU).
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "closure_terms.hpp"

namespace cyc {

inline uint64_t zone_words(uint64_t Z) { return (Z + 63) / 64; }             // Wz: words of a row of the zone plane
inline uint64_t zone_pitch(uint64_t Z) { return closure_pitch(zone_words(Z)); }  // of the scratch planes: whole lines

// cyc_table_zone_graph's arguments that can be judged before anything runs; nullptr when they are fine
inline const char* zone_graph_args_bad(const void* n_zones, const void* edges, int64_t edge_cap, const void* n_edges, const void* d_zreach,
                                       int64_t zreach_words) {
  if (!n_zones) return "null n_zones";
  if (edge_cap < 0) return "negative edge_cap";
  if (!edges && edge_cap > 0) return "null edges with edge_cap > 0";
  if (edges && !n_edges) return "edges without n_edges";
  if (reinterpret_cast<uintptr_t>(d_zreach) % 8) return "d_zreach is not 8-byte aligned";
  if (d_zreach && zreach_words < 0) return "negative zreach_words";
  return nullptr;
}

// the two capacity failures (`why` holds the built message)
inline const char* zone_zreach_cap_bad(int64_t zreach_words, int64_t Z, std::string& why) {
  const uint64_t need = uint64_t(Z) * zone_words(uint64_t(Z));
  if (uint64_t(zreach_words) >= need) return nullptr;
  why = "zreach_words = " + std::to_string(zreach_words) + " is less than the " + std::to_string(need) + " words of the plane of " +
        std::to_string(Z) + " zones";
  return why.c_str();
}
inline const char* zone_edge_cap_bad(int64_t edge_cap, uint64_t total, std::string& why) {
  if (uint64_t(edge_cap) >= total) return nullptr;
  why = "edge_cap = " + std::to_string(edge_cap) + " is less than the " + std::to_string(total) + " cover edges";
  return why.c_str();
}

// The zones' smallest pods in ascending order (rep as checked by zone_reps_bad): zone z is the z-th of them.
inline void zone_heads(const uint32_t* rep, int64_t P, std::vector<uint32_t>& head) {
  head.clear();
  for (int64_t p = 0; p < P; p++)
    if (int64_t(rep[p]) == p) head.push_back(uint32_t(p));
}

// size[z]: the pods of zone z (zone ids in [0, Z))
inline void zone_sizes(const int32_t* zone, int64_t P, int64_t Z, std::vector<int64_t>& size) {
  size.assign(size_t(Z), 0);
  for (int64_t p = 0; p < P; p++) size[size_t(zone[p])]++;
}

// Exclusive scan of the rows' edge counts, in place; returns the total.
inline uint64_t zone_offsets(unsigned long long* cnt, int64_t Z) {
  uint64_t at = 0;
  for (int64_t z = 0; z < Z; z++) {
    const uint64_t n = cnt[z];
    cnt[z] = at, at += n;
  }
  return at;
}

// The edge list the device delivers: both ends in [0, Z), a != b, ascending (a, b) without repeats.  nullptr when it is
// fine; anything else means the cover plane was not one.
inline const char* zone_edges_bad(const cyc_zone_edge* e, int64_t n, int64_t Z, std::string& why) {
  for (int64_t i = 0; i < n; i++) {
    const bool in = e[i].a >= 0 && e[i].a < Z && e[i].b >= 0 && e[i].b < Z && e[i].a != e[i].b;
    const bool up = i == 0 || e[i - 1].a < e[i].a || (e[i - 1].a == e[i].a && e[i - 1].b < e[i].b);
    if (!in || !up) {
      why = "internal: edge " + std::to_string(i) + " = (" + std::to_string(e[i].a) + ", " + std::to_string(e[i].b) + ") " +
            (in ? "is out of order" : "is not an edge between two of the " + std::to_string(Z) + " zones");
      return why.c_str();
    }
  }
  return nullptr;
}

// tier[z]: the edges of the longest chain of edges that ends in z, by Kahn's pass over the list (as checked by
// zone_edges_bad: sorted by a).  A zone that is left over sits on a cycle, which a strict partial order has none of:
// nullptr when there is none.
inline const char* zone_tiers(const cyc_zone_edge* e, int64_t n, int64_t Z, std::vector<int32_t>& tier, std::string& why) {
  tier.assign(size_t(Z), 0);
  std::vector<int64_t> start(size_t(Z) + 1, 0), waits(size_t(Z), 0);
  for (int64_t i = 0; i < n; i++) start[size_t(e[i].a) + 1]++, waits[size_t(e[i].b)]++;
  for (int64_t z = 0; z < Z; z++) start[size_t(z) + 1] += start[size_t(z)];
  std::vector<int32_t> ready;
  ready.reserve(size_t(Z));
  for (int64_t z = 0; z < Z; z++)
    if (!waits[size_t(z)]) ready.push_back(int32_t(z));
  for (size_t at = 0; at < ready.size(); at++) {
    const int32_t a = ready[at];
    for (int64_t i = start[size_t(a)]; i < start[size_t(a) + 1]; i++) {
      const int32_t b = e[i].b;
      if (tier[size_t(b)] < tier[size_t(a)] + 1) tier[size_t(b)] = tier[size_t(a)] + 1;
      if (!--waits[size_t(b)]) ready.push_back(b);
    }
  }
  if (int64_t(ready.size()) == Z) return nullptr;
  for (int64_t z = 0; z < Z; z++)
    if (waits[size_t(z)]) {
      why = "internal: zone " + std::to_string(z) + " lies on a cycle of cover edges";
      break;
    }
  return why.c_str();
}

}  // namespace cyc
