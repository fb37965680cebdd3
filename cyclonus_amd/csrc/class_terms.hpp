// class_terms.hpp — the host arithmetic of cyc_table_classes and cyc_table_cells_at (classes.hpp) that is not a
// launch: the checks of the pod lists, the destinations' status keys, the grouping of the pods by (masked hash, status
// key), the election of new representatives among the pods that failed a verification, and the canonical numbering.
// Plain integer C++ without HIP (tests/native/class_terms_check.cpp runs it on the CPU).
#pragma once

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "table_terms.hpp"

namespace cyc {

// A pod list of cyc_table_cells_at; nullptr when it is fine (`why` holds a built message).  Nothing behind this
// indexes by an entry that it has not seen.
inline const char* pod_list_bad(int64_t P, const char* name, const int32_t* list, int64_t n, std::string& why) {
  if (n < 0) return why = std::string("negative count of ") + name, why.c_str();
  if (n > 0 && !list) return why = std::string("null ") + name, why.c_str();
  for (int64_t i = 0; i < n; i++)
    if (list[i] < 0 || list[i] >= P) {
      why = std::string(name) + "[" + std::to_string(i) + "] = " + std::to_string(list[i]) + " is not a pod in [0, " + std::to_string(P) + ")";
      return why.c_str();
    }
  return nullptr;
}

// What a destination's statuses contribute to its column of codes in `view`, a byte per slot of the range: VALID is a
// value of its own (the plane bits decide there), any other status counts as the code it gives every cell of (d, k).
constexpr uint8_t CLASS_KEY_VALID = 0xFE;  // (no cyc_connectivity code: CYC_CONN_NO_JOB is 0xFF)
inline void class_status_keys(int view, const uint8_t* st, int64_t P, int64_t K, int64_t k_lo, int64_t nk, std::vector<uint8_t>& keys) {
  keys.assign(size_t(P * nk), 0);
  for (int64_t d = 0; d < P; d++)
    for (int64_t kk = 0; kk < nk; kk++) {
      const uint8_t s = status_norm(st[d * K + k_lo + kk]);
      keys[size_t(d * nk + kk)] = s == CYC_JOB_VALID ? CLASS_KEY_VALID : uint8_t(status_code(view, s));
    }
}

// The pods of one side on their way to classes.  start() groups them by key = (h & mask, the pod's nkey key bytes,
// compared exactly); the candidate representative of a pod is the smallest pod with its key, and every other pod is
// listed for verification against it.  The caller then sets bad[i] for the listed pods whose rows differ from their
// representative's and calls refine(): the pods that passed are settled; within each key group the pods that failed
// elect their smallest member, which is settled as a representative, and the others are listed against it.  Every
// round settles at least one pod per group that is still listed, so the rounds end, and since only equal rows settle
// together the result is exact whatever h holds.  Rows that are equal have equal keys (h is a function of the row),
// so in the end rep[p] is the smallest pod of p's class.
struct ClassRounds {
  std::vector<int32_t> rep;          // [P]
  std::vector<uint32_t> pod, cand;   // the list: pod[i] is to be compared with cand[i] == rep[pod[i]], pods ascending
  int64_t rounds = 0, failed = 0;    // verifications asked for; pods that failed one

  void start(int64_t P, const uint64_t* h, uint64_t mask, const uint8_t* keys, int64_t nkey) {
    rep.assign(size_t(P), 0), group.assign(size_t(P), 0), elect.assign(size_t(P), -1);
    std::vector<int32_t> order(size_t(P), 0);
    for (int64_t p = 0; p < P; p++) order[size_t(p)] = int32_t(p);
    auto key_cmp = [&](int32_t x, int32_t y) {
      return keys && nkey ? std::lexicographical_compare(keys + x * nkey, keys + (x + 1) * nkey, keys + y * nkey, keys + (y + 1) * nkey) : false;
    };
    std::sort(order.begin(), order.end(), [&](int32_t x, int32_t y) {
      const uint64_t hx = h[x] & mask, hy = h[y] & mask;
      if (hx != hy) return hx < hy;
      if (key_cmp(x, y)) return true;
      if (key_cmp(y, x)) return false;
      return x < y;
    });
    for (size_t i = 0; i < order.size(); i++) {
      const int32_t p = order[i], q = i ? order[i - 1] : -1;
      const bool same = i && (h[p] & mask) == (h[q] & mask) && !key_cmp(p, q) && !key_cmp(q, p);
      group[size_t(p)] = same ? group[size_t(q)] : p;  // (the group's smallest pod names it)
    }
    for (int64_t p = 0; p < P; p++) rep[size_t(p)] = group[size_t(p)];
    relist();
  }
  bool done() const { return pod.empty(); }
  // bad: [pod.size()], non-zero where the rows of pod[i] and cand[i] differ
  void refine(const uint32_t* bad) {
    rounds++;
    for (size_t i = 0; i < pod.size(); i++) {
      if (!bad[i]) continue;
      failed++;
      int32_t& e = elect[size_t(group[pod[i]])];
      if (e < 0) e = int32_t(pod[i]);  // (the list is ascending: the first is the smallest)
      rep[pod[i]] = e;
    }
    for (size_t i = 0; i < pod.size(); i++) elect[size_t(group[pod[i]])] = -1;
    std::vector<uint32_t> next;
    for (size_t i = 0; i < pod.size(); i++)
      if (bad[i] && rep[pod[i]] != int32_t(pod[i])) next.push_back(pod[i]);
    pod.swap(next);
    cand.resize(pod.size());
    for (size_t i = 0; i < pod.size(); i++) cand[i] = uint32_t(rep[pod[i]]);
  }
  // Canonical class ids from the settled representatives: 0, 1, ... in the order of the classes' smallest pods.
  // cls: [P] or null.  Returns the number of classes.
  int64_t number(int32_t* cls) const {
    std::vector<int32_t> id(rep.size(), 0);
    int32_t n = 0;
    for (size_t p = 0; p < rep.size(); p++) {
      id[p] = rep[p] == int32_t(p) ? n++ : id[size_t(rep[p])];  // (rep[p] <= p)
      if (cls) cls[p] = id[p];
    }
    return n;
  }

 private:
  std::vector<int32_t> group, elect;  // the smallest pod of the pod's key group; per group, this round's elected pod
  void relist() {
    pod.clear(), cand.clear();
    for (size_t p = 0; p < rep.size(); p++)
      if (rep[p] != int32_t(p)) pod.push_back(uint32_t(p)), cand.push_back(uint32_t(rep[p]));
  }
};

}  // namespace cyc
