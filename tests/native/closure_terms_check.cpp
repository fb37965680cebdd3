// closure_terms_check.cpp — the host arithmetic of cyc_table_closure / cyc_table_zones
// (cyclonus_amd/csrc/closure_terms.hpp) on the CPU: the argument messages, the scratch pitch, the check of the
// representatives (a representative above its pod, one that is not its own, one beyond P) and the canonical numbering
// against zones found here pair by pair on random digraphs closed by plain Warshall.
// Built with g++ under ASan + UBSan and run by tests/test_closure_terms.py; exits non-zero on a mismatch.
#include <cstdio>
#include <string>
#include <vector>

#include "closure_terms.hpp"

using namespace cyc;

static int failures = 0;
static std::string ctx;
static void expect(bool ok, const char* what, int line) {
  if (!ok && failures++ < 25) std::printf("line %d: %s: %s\n", line, ctx.c_str(), what);
}
#define EXPECT(c) expect((c), #c, __LINE__)
#define SAME(got, want) expect((got) == (want), #got " != " #want, __LINE__)

static uint64_t rng = 1;
static uint32_t rnd() {
  rng ^= rng << 13, rng ^= rng >> 7, rng ^= rng << 17;
  return uint32_t(rng >> 24);
}

static std::string str(const char* m) { return m ? std::string(m) : std::string(); }

static void check_arguments() {
  ctx = "arguments";
  alignas(16) uint64_t plane[4];
  int64_t n[1];
  char* p = reinterpret_cast<char*>(plane);
  SAME(str(closure_outputs_bad(p, n)), "");
  SAME(str(closure_outputs_bad(p + 8, nullptr)), "");  // (8-byte alignment is enough)
  SAME(str(closure_outputs_bad(nullptr, n)), "");
  SAME(str(closure_outputs_bad(nullptr, nullptr)), "no output requested");
  for (int off : {1, 2, 4, 7, 12}) SAME(str(closure_outputs_bad(p + off, n)), "d_closure is not 8-byte aligned");
  SAME(str(closure_outputs_bad(p + 4, nullptr)), "d_closure is not 8-byte aligned");
  SAME(str(zones_outputs_bad(nullptr, nullptr, nullptr, nullptr)), "no output requested");
  for (int x = 0; x < 4; x++) SAME(str(zones_outputs_bad(x == 0 ? n : nullptr, x == 1 ? n : nullptr, x == 2 ? n : nullptr, x == 3 ? n : nullptr)), "");
  SAME(closure_pitch(0), 0u);
  SAME(closure_pitch(1), 16u);
  SAME(closure_pitch(16), 16u);
  SAME(closure_pitch(17), 32u);
  SAME(closure_pitch(1563), 1568u);
}

static std::string reps_bad(const std::vector<uint32_t>& rep) {
  std::string why;
  return str(zone_reps_bad(rep.data(), int64_t(rep.size()), why));
}

static void check_reps() {
  ctx = "representatives";
  SAME(reps_bad({}), "");
  SAME(reps_bad({0}), "");
  SAME(reps_bad({0, 0, 2, 0, 2}), "");
  SAME(reps_bad({0, 2, 2}), "internal: rep[1] = 2 is not the smallest pod of a zone");
  SAME(reps_bad({0, 0, 1}), "internal: rep[2] = 1 is not the smallest pod of a zone");
  SAME(reps_bad({1}), "internal: rep[0] = 1 is not the smallest pod of a zone");
  SAME(reps_bad({0, 1, 0xFFFFFFFFu}), "internal: rep[2] = 4294967295 is not the smallest pod of a zone");
  std::vector<int32_t> id{9}, zone(5, -1);
  const std::vector<uint32_t> rep{0, 0, 2, 0, 2};
  SAME(zone_number(rep.data(), 5, zone.data(), id), int64_t(2));
  SAME(zone, (std::vector<int32_t>{0, 0, 1, 0, 1}));
  SAME(id, zone);
  SAME(zone_number(rep.data(), 5, nullptr, id), int64_t(2));  // (the count alone)
  SAME(zone_number(rep.data(), 0, nullptr, id), int64_t(0));
  EXPECT(id.empty());
}

// random digraph -> Warshall -> rep by the definition -> the numbering against one found pair by pair
static void check_numbering(int P, int edges) {
  ctx = "numbering P " + std::to_string(P) + " edges " + std::to_string(edges);
  std::vector<char> r(size_t(P) * P, 0);
  for (int p = 0; p < P; p++) r[size_t(p) * P + p] = 1;
  for (int i = 0; i < edges; i++) r[size_t(rnd() % P) * P + rnd() % P] = 1;
  for (int k = 0; k < P; k++)
    for (int i = 0; i < P; i++)
      if (r[size_t(i) * P + k])
        for (int j = 0; j < P; j++) r[size_t(i) * P + j] |= r[size_t(k) * P + j];
  std::vector<uint32_t> rep(size_t(P), 0);
  for (int p = 0; p < P; p++)
    for (int q = 0; q < P; q++)
      if (r[size_t(p) * P + q] && r[size_t(q) * P + p]) {
        rep[size_t(p)] = uint32_t(q);
        break;
      }
  SAME(reps_bad(rep), "");
  std::vector<int32_t> zone(size_t(P), -7), id;
  const int64_t n = zone_number(rep.data(), P, zone.data(), id);
  // by the definition: a new id for every pod that shares a zone with no smaller pod
  int64_t want_n = 0;
  std::vector<int32_t> want(size_t(P), -1);
  for (int p = 0; p < P; p++) {
    for (int q = 0; q < p && want[size_t(p)] < 0; q++)
      if (r[size_t(p) * P + q] && r[size_t(q) * P + p]) want[size_t(p)] = want[size_t(q)];
    if (want[size_t(p)] < 0) want[size_t(p)] = int32_t(want_n++);
  }
  SAME(n, want_n);
  SAME(zone, want);
  if (P) SAME(zone[0], 0);
}

int main() {
  check_arguments();
  check_reps();
  for (int P : {1, 2, 63, 64, 65, 200})
    for (int per_pod : {0, 1, 2}) check_numbering(P, per_pod * P + per_pod * P / 3);
  if (failures) return std::printf("closure terms: %d failures\n", failures), 1;
  std::printf("closure terms: ok\n");
  return 0;
}
