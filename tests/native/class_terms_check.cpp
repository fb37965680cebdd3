// class_terms_check.cpp — the host arithmetic of cyc_table_classes / cyc_table_cells_at (cyclonus_amd/csrc/class_terms.hpp)
// on the CPU: the grouping by (masked hash, status key), the election among the pods that failed a verification over
// several rounds and the first-occurrence numbering, with the device's verification simulated on rows written out here;
// for the masks ~0, 0xF and 0 and for hashes that are good, constant or wrong (equal for unequal rows) the classes
// must be those of a pairwise comparison of the rows and keys.  Then the status keys per view and the messages of the
// list checks.  Built with g++ under ASan + UBSan and run by tests/test_class_terms.py; exits non-zero on a mismatch.
#include <cstdio>
#include <string>
#include <vector>

#include "class_terms.hpp"

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

using Rows = std::vector<std::vector<uint64_t>>;

// the classes by comparing every pod with every earlier one: row and key bytes equal
static std::vector<int32_t> pairwise(const Rows& rows, const std::vector<uint8_t>& keys, int64_t nkey, int64_t& n) {
  const size_t P = rows.size();
  std::vector<int32_t> cls(P, -1);
  n = 0;
  for (size_t p = 0; p < P; p++) {
    for (size_t q = 0; q < p && cls[p] < 0; q++)
      if (rows[p] == rows[q] && std::equal(keys.begin() + p * nkey, keys.begin() + (p + 1) * nkey, keys.begin() + q * nkey)) cls[p] = cls[q];
    if (cls[p] < 0) cls[p] = int32_t(n++);
  }
  return cls;
}

static uint64_t row_hash(const std::vector<uint64_t>& row) {
  uint64_t h = 1469598103934665603ull;
  for (uint64_t w : row) h = (h ^ w) * 1099511628211ull;
  return h;
}

// the two phases as classes.hpp runs them, the verification done here
static std::vector<int32_t> run(const Rows& rows, const std::vector<uint64_t>& h, uint64_t mask, const std::vector<uint8_t>& keys, int64_t nkey,
                                int64_t& n, ClassRounds& r) {
  const int64_t P = int64_t(rows.size());
  r.start(P, h.data(), mask, nkey ? keys.data() : nullptr, nkey);
  int64_t rounds = 0;
  while (!r.done()) {
    EXPECT(r.pod.size() == r.cand.size());
    std::vector<uint32_t> bad(r.pod.size());
    for (size_t i = 0; i < r.pod.size(); i++) {
      EXPECT(r.cand[i] < r.pod[i] && (i == 0 || r.pod[i - 1] < r.pod[i]));
      bad[i] = rows[r.pod[i]] != rows[r.cand[i]];
    }
    r.refine(bad.data());
    EXPECT(++rounds <= P);  // (every round settles a pod)
  }
  SAME(r.rounds, rounds);
  std::vector<int32_t> cls(size_t(P), -7);
  n = r.number(cls.data());
  SAME(r.number(nullptr), n);
  return cls;
}

static void check_classes() {
  for (int64_t P : {0, 1, 2, 7, 64, 65, 200})
    for (int64_t words : {1, 3})
      for (int64_t nkey : {0, 2})
        for (int variety : {1, 3, 12}) {
          Rows rows(size_t(P), std::vector<uint64_t>(size_t(words), 0));
          std::vector<uint8_t> keys(size_t(P * nkey), 0);
          for (auto& row : rows) {
            const uint32_t v = rnd() % uint32_t(variety);
            for (int64_t w = 0; w < words; w++) row[size_t(w)] = v * 0x9E3779B97F4A7C15ull + uint64_t(w) * (v + 1);
          }
          for (auto& x : keys) x = rnd() % 8 ? CLASS_KEY_VALID : uint8_t(rnd() % 3);
          int64_t want_n = 0;
          const std::vector<int32_t> want = pairwise(rows, keys, nkey, want_n);
          for (int kind = 0; kind < 3; kind++) {
            // hashes: of the row; the same for every pod; of the row's first word alone (equal for some unequal rows)
            std::vector<uint64_t> h(static_cast<size_t>(P), 0);
            for (int64_t p = 0; p < P; p++) h[size_t(p)] = kind == 0 ? row_hash(rows[size_t(p)]) : kind == 1 ? 42 : rows[size_t(p)][0] % 3;
            for (uint64_t mask : {~0ull, 0xFull, 0ull}) {
              ctx = "P " + std::to_string(P) + " words " + std::to_string(words) + " nkey " + std::to_string(nkey) + " variety " +
                    std::to_string(variety) + " hash kind " + std::to_string(kind) + " mask " + std::to_string(mask);
              int64_t n = -1;
              ClassRounds r;
              const std::vector<int32_t> got = run(rows, h, mask, keys, nkey, n, r);
              SAME(n, want_n);
              EXPECT(got == want);
              if (P) SAME(got[0], 0);
              if (kind == 0 && mask == ~0ull) {
                SAME(r.failed, int64_t(0));
                EXPECT(r.rounds <= 1);
              }
              // without the keys, a constant hash leaves everything to the verification: a round per class, but none for
              // a last class of one pod; every pod outside the first class failed at least once
              if (kind == 1 && nkey == 0 && P) {
                EXPECT(r.rounds >= want_n - 1 && r.rounds <= want_n);
                EXPECT(r.failed >= want_n - 1);
              }
            }
          }
        }
}

static void check_election() {
  // one key group, rows A B A C B C C: round 1 compares all with pod 0, round 2 the failed with pod 1, round 3 with pod 3
  ctx = "election";
  const Rows rows{{1}, {2}, {1}, {3}, {2}, {3}, {3}};
  const std::vector<uint64_t> h(7, 5);
  ClassRounds r;
  r.start(7, h.data(), ~0ull, nullptr, 0);
  EXPECT((r.pod == std::vector<uint32_t>{1, 2, 3, 4, 5, 6}) && (r.cand == std::vector<uint32_t>(6, 0)));
  const uint32_t bad1[] = {1, 0, 1, 1, 1, 1};
  r.refine(bad1);
  EXPECT((r.pod == std::vector<uint32_t>{3, 4, 5, 6}) && (r.cand == std::vector<uint32_t>(4, 1)));
  const uint32_t bad2[] = {1, 0, 1, 1};
  r.refine(bad2);
  EXPECT((r.pod == std::vector<uint32_t>{5, 6}) && (r.cand == std::vector<uint32_t>(2, 3)));
  const uint32_t bad3[] = {0, 0};
  r.refine(bad3);
  EXPECT(r.done());
  SAME(r.rounds, int64_t(3));
  SAME(r.failed, int64_t(5 + 3));
  std::vector<int32_t> cls(7);
  SAME(r.number(cls.data()), int64_t(3));
  EXPECT((cls == std::vector<int32_t>{0, 1, 0, 2, 1, 2, 2}));
  // two key groups elect independently in the same round: hashes 0 1 0 1 0 1, rows A B C D C D
  const Rows rows2{{1}, {2}, {3}, {4}, {3}, {4}};
  const std::vector<uint64_t> h2{0, 1, 0, 1, 0, 1};
  ClassRounds q;
  q.start(6, h2.data(), 1, nullptr, 0);
  EXPECT((q.pod == std::vector<uint32_t>{2, 3, 4, 5}) && (q.cand == std::vector<uint32_t>{0, 1, 0, 1}));
  const uint32_t bad4[] = {1, 1, 1, 1};
  q.refine(bad4);
  EXPECT((q.pod == std::vector<uint32_t>{4, 5}) && (q.cand == std::vector<uint32_t>{2, 3}));
  const uint32_t bad5[] = {0, 0};
  q.refine(bad5);
  EXPECT(q.done());
  SAME(q.number(cls.data()), int64_t(4));
  (void)rows2;
}

static void check_status_keys() {
  ctx = "status keys";
  // P 2, K 4: pod 0 VALID NONE BNP BPP, pod 1 BPP BNP VALID 9 (outside cyc_job_status: counted as BAD_NAMED_PORT)
  const uint8_t st[] = {CYC_JOB_VALID, CYC_JOB_NONE, CYC_JOB_BAD_NAMED_PORT, CYC_JOB_BAD_PORT_PROTOCOL,
                        CYC_JOB_BAD_PORT_PROTOCOL, CYC_JOB_BAD_NAMED_PORT, CYC_JOB_VALID, 9};
  std::vector<uint8_t> k;
  class_status_keys(CYC_VIEW_INGRESS, st, 2, 4, 0, 4, k);
  const uint8_t np = CYC_CONN_INVALID_NAMED_PORT, pp = CYC_CONN_INVALID_PORT_PROTOCOL, nj = CYC_CONN_NO_JOB, un = CYC_CONN_UNKNOWN;
  EXPECT((k == std::vector<uint8_t>{CLASS_KEY_VALID, nj, np, pp, pp, np, CLASS_KEY_VALID, np}));
  class_status_keys(CYC_VIEW_COMBINED, st, 2, 4, 1, 3, k);
  EXPECT((k == std::vector<uint8_t>{nj, np, pp, np, CLASS_KEY_VALID, np}));
  class_status_keys(CYC_VIEW_EGRESS, st, 2, 4, 0, 4, k);
  EXPECT((k == std::vector<uint8_t>{CLASS_KEY_VALID, nj, un, un, un, un, CLASS_KEY_VALID, un}));
  class_status_keys(CYC_VIEW_EGRESS, st, 2, 4, 2, 0, k);
  EXPECT(k.empty());
  EXPECT(CLASS_KEY_VALID != nj && CLASS_KEY_VALID > 5);  // (no code is the VALID value)
}

static std::string bad(int64_t P, const char* name, const std::vector<int32_t>& list, int64_t n, bool null = false) {
  std::string why;
  const char* m = pod_list_bad(P, name, null ? nullptr : list.data(), n, why);
  return m ? std::string(m) : std::string();
}

static void check_lists() {
  ctx = "lists";
  SAME(bad(65, "srcs", {3, 0, 64, 3}, 4), "");
  SAME(bad(65, "srcs", {}, 0, true), "");
  SAME(bad(65, "srcs", {}, -1), "negative count of srcs");
  SAME(bad(65, "dsts", {}, -5, true), "negative count of dsts");
  SAME(bad(65, "dsts", {}, 2, true), "null dsts");
  SAME(bad(65, "srcs", {65, 0, 1}, 3), "srcs[0] = 65 is not a pod in [0, 65)");
  SAME(bad(65, "dsts", {0, -1, 70}, 3), "dsts[1] = -1 is not a pod in [0, 65)");
  SAME(bad(65, "dsts", {0, 1, 2147483647}, 3), "dsts[2] = 2147483647 is not a pod in [0, 65)");
  SAME(bad(0, "srcs", {0}, 1), "srcs[0] = 0 is not a pod in [0, 0)");
}

int main() {
  check_classes();
  check_election();
  check_status_keys();
  check_lists();
  if (failures) return std::printf("class terms: %d failures\n", failures), 1;
  std::printf("class terms: ok\n");
  return 0;
}
