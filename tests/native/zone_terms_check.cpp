// zone_terms_check.cpp — the host arithmetic of cyc_table_zone_graph (cyclonus_amd/csrc/zone_terms.hpp) on the CPU: the
// argument and capacity messages, the plane sizes, the zones' smallest pods and sizes, the offsets, the check of the edge
// list (an end outside [0, Z), a loop, a repeat, a descent) and the tiers against the longest chains found here by
// relaxing random DAGs to a fixed point; a cycle is reported.
// Built with g++ under ASan + UBSan and run by tests/test_zone_terms.py; exits non-zero on a mismatch.
#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "zone_terms.hpp"

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
  cyc_zone_edge e[1];
  char* p = reinterpret_cast<char*>(plane);
  SAME(str(zone_graph_args_bad(n, e, 1, n, p, 4)), "");
  SAME(str(zone_graph_args_bad(n, nullptr, 0, nullptr, nullptr, 0)), "");  // (the smallest call: Z alone)
  SAME(str(zone_graph_args_bad(n, nullptr, 0, n, nullptr, 0)), "");        // (count-only)
  SAME(str(zone_graph_args_bad(n, e, 0, n, p + 8, 0)), "");                // (8-byte alignment is enough)
  SAME(str(zone_graph_args_bad(nullptr, e, 1, n, p, 4)), "null n_zones");
  SAME(str(zone_graph_args_bad(n, e, -1, n, p, 4)), "negative edge_cap");
  SAME(str(zone_graph_args_bad(n, nullptr, 1, n, p, 4)), "null edges with edge_cap > 0");
  SAME(str(zone_graph_args_bad(n, e, 1, nullptr, p, 4)), "edges without n_edges");
  for (int off : {1, 2, 4, 7, 12}) SAME(str(zone_graph_args_bad(n, e, 1, n, p + off, 4)), "d_zreach is not 8-byte aligned");
  SAME(str(zone_graph_args_bad(n, e, 1, n, p, -1)), "negative zreach_words");
  SAME(str(zone_graph_args_bad(n, e, 1, n, nullptr, -1)), "");
  SAME(zone_words(0), 0u);
  SAME(zone_words(1), 1u);
  SAME(zone_words(64), 1u);
  SAME(zone_words(65), 2u);
  SAME(zone_pitch(0), 0u);
  SAME(zone_pitch(1), 16u);
  SAME(zone_pitch(1024), 16u);
  SAME(zone_pitch(1025), 32u);
  std::string why;
  SAME(str(zone_zreach_cap_bad(130, 65, why)), "");
  SAME(str(zone_zreach_cap_bad(129, 65, why)), "zreach_words = 129 is less than the 130 words of the plane of 65 zones");
  SAME(str(zone_zreach_cap_bad(0, 1, why)), "zreach_words = 0 is less than the 1 words of the plane of 1 zones");
  SAME(str(zone_zreach_cap_bad(0, 0, why)), "");
  SAME(str(zone_edge_cap_bad(3, 3, why)), "");
  SAME(str(zone_edge_cap_bad(0, 0, why)), "");
  SAME(str(zone_edge_cap_bad(2, 3, why)), "edge_cap = 2 is less than the 3 cover edges");
}

static void check_heads_sizes_offsets() {
  ctx = "heads, sizes, offsets";
  const uint32_t rep[] = {0, 0, 2, 0, 2, 5};
  std::vector<uint32_t> head;
  zone_heads(rep, 6, head);
  SAME(head, (std::vector<uint32_t>{0, 2, 5}));
  std::vector<int32_t> id;
  int32_t zone[6];
  SAME(zone_number(rep, 6, zone, id), 3);
  std::vector<int64_t> size;
  zone_sizes(zone, 6, 3, size);
  SAME(size, (std::vector<int64_t>{3, 2, 1}));
  zone_heads(rep, 0, head);
  EXPECT(head.empty());
  zone_sizes(zone, 0, 0, size);
  EXPECT(size.empty());
  unsigned long long cnt[] = {2, 0, 3, 1};
  SAME(zone_offsets(cnt, 4), 6u);
  SAME(std::vector<unsigned long long>(cnt, cnt + 4), (std::vector<unsigned long long>{0, 2, 2, 5}));
  SAME(zone_offsets(cnt, 0), 0u);
}

static void check_edge_lists() {
  ctx = "edge lists";
  std::string why;
  const cyc_zone_edge good[] = {{0, 1}, {0, 3}, {1, 2}, {3, 2}};
  SAME(str(zone_edges_bad(good, 4, 4, why)), "");
  SAME(str(zone_edges_bad(good, 0, 0, why)), "");
  const cyc_zone_edge loop[] = {{0, 1}, {1, 1}};
  SAME(str(zone_edges_bad(loop, 2, 4, why)), "internal: edge 1 = (1, 1) is not an edge between two of the 4 zones");
  const cyc_zone_edge far[] = {{0, 4}};
  SAME(str(zone_edges_bad(far, 1, 4, why)), "internal: edge 0 = (0, 4) is not an edge between two of the 4 zones");
  const cyc_zone_edge neg[] = {{-1, 2}};
  SAME(str(zone_edges_bad(neg, 1, 4, why)), "internal: edge 0 = (-1, 2) is not an edge between two of the 4 zones");
  const cyc_zone_edge twice[] = {{0, 1}, {0, 1}};
  SAME(str(zone_edges_bad(twice, 2, 4, why)), "internal: edge 1 = (0, 1) is out of order");
  const cyc_zone_edge down[] = {{2, 1}, {1, 3}};
  SAME(str(zone_edges_bad(down, 2, 4, why)), "internal: edge 1 = (1, 3) is out of order");
}

static void check_tiers() {
  std::string why;
  std::vector<int32_t> tier;
  ctx = "tiers by hand";
  const cyc_zone_edge diamond[] = {{0, 1}, {0, 2}, {1, 3}, {2, 3}};
  SAME(str(zone_tiers(diamond, 4, 5, tier, why)), "");
  SAME(tier, (std::vector<int32_t>{0, 1, 1, 2, 0}));
  SAME(str(zone_tiers(diamond, 0, 0, tier, why)), "");
  EXPECT(tier.empty());
  const cyc_zone_edge cycle[] = {{0, 1}, {1, 2}, {2, 1}};
  SAME(str(zone_tiers(cycle, 3, 4, tier, why)), "internal: zone 1 lies on a cycle of cover edges");
  const cyc_zone_edge up[] = {{1, 0}, {2, 1}, {3, 2}};  // (a chain against the numbering)
  SAME(str(zone_tiers(up, 3, 4, tier, why)), "");
  SAME(tier, (std::vector<int32_t>{3, 2, 1, 0}));
  for (int round = 0; round < 200; round++) {
    ctx = "tiers of random DAG " + std::to_string(round);
    const int64_t Z = 1 + rnd() % 40;
    // a DAG along a random order of the zones, as a sorted list without repeats
    std::vector<int32_t> place(static_cast<size_t>(Z));
    for (int64_t z = 0; z < Z; z++) place[size_t(z)] = int32_t(z);
    for (int64_t z = Z - 1; z > 0; z--) std::swap(place[size_t(z)], place[rnd() % (z + 1)]);
    std::vector<cyc_zone_edge> e;
    for (int32_t a = 0; a < Z; a++)
      for (int32_t b = 0; b < Z; b++)
        if (place[size_t(a)] < place[size_t(b)] && rnd() % 6 == 0) e.push_back({a, b});
    SAME(str(zone_edges_bad(e.data(), int64_t(e.size()), Z, why)), "");
    SAME(str(zone_tiers(e.data(), int64_t(e.size()), Z, tier, why)), "");
    std::vector<int32_t> want(static_cast<size_t>(Z), 0);
    for (bool moved = true; moved;) {
      moved = false;
      for (const cyc_zone_edge& x : e)
        if (want[size_t(x.b)] < want[size_t(x.a)] + 1) want[size_t(x.b)] = want[size_t(x.a)] + 1, moved = true;
    }
    SAME(tier, want);
    if (!e.empty()) {  // the back edge of one of them closes a cycle
      std::vector<cyc_zone_edge> c = e;
      c.push_back({e[0].b, e[0].a});
      std::sort(c.begin(), c.end(), [](const cyc_zone_edge& x, const cyc_zone_edge& y) { return x.a != y.a ? x.a < y.a : x.b < y.b; });
      EXPECT(str(zone_tiers(c.data(), int64_t(c.size()), Z, tier, why)).find("lies on a cycle of cover edges") != std::string::npos);
    }
  }
}

int main() {
  check_arguments();
  check_heads_sizes_offsets();
  check_edge_lists();
  check_tiers();
  if (failures) return std::printf("zone terms: %d failures\n", failures), 1;
  std::printf("zone terms: ok\n");
  return 0;
}
