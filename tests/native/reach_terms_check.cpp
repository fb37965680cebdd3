// reach_terms_check.cpp — the host arithmetic of cyc_table_reach (cyclonus_amd/csrc/reach_terms.hpp) on the CPU:
// the seed checks and their messages (bad seeds first, last and in the middle; bad seed_off), the seed lists as
// bitsets against a per-pod tally (empty sets, duplicates, P at 1, 64 and 65 and beyond), the working-set limit at
// its edge, and `levels` from the counters of a search done here pod by pod.
// Built with g++ under ASan + UBSan and run by tests/test_reach_terms.py; exits non-zero on a mismatch.
#include <cstdio>
#include <string>
#include <vector>

#include "reach_terms.hpp"

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

static std::string bad(int64_t P, const std::vector<int64_t>& off, const std::vector<int32_t>& seeds, int64_t n_sets,
                       bool null_off = false, bool null_seeds = false) {
  std::string why;
  const char* m = reach_seeds_bad(P, null_off ? nullptr : off.data(), null_seeds ? nullptr : seeds.data(), n_sets, why);
  return m ? std::string(m) : std::string();
}

static void check_refusals() {
  ctx = "refusals";
  const std::vector<int64_t> off{0, 2, 2, 5};
  const std::vector<int32_t> good{3, 0, 64, 3, 1};
  SAME(bad(65, off, good, 3), "");
  SAME(bad(65, off, good, -1), "negative n_sets");
  SAME(bad(65, off, good, 3, true), "null seed_off");
  SAME(bad(65, off, good, 3, false, true), "null seeds");
  SAME(bad(65, {0, 0, 0, 0}, {}, 3, false, true), "");  // (no seed at all: seeds is not read)
  SAME(bad(65, {0}, {}, 0, false, true), "");
  SAME(bad(65, {1, 2, 2, 5}, good, 3), "seed_off must start at 0 and never decrease");
  SAME(bad(65, {0, 2, 1, 5}, good, 3), "seed_off must start at 0 and never decrease");
  SAME(bad(65, {0, 2, 2, 1}, good, 3), "seed_off must start at 0 and never decrease");
  // a bad seed first, in the middle and last; the first bad one is named; both sides of the range
  SAME(bad(65, off, {65, 0, 64, 3, 1}, 3), "seeds[0] = 65 is not a pod in [0, 65)");
  SAME(bad(65, off, {3, 0, -1, 3, 1}, 3), "seeds[2] = -1 is not a pod in [0, 65)");
  SAME(bad(65, off, {3, 0, 64, 3, 70}, 3), "seeds[4] = 70 is not a pod in [0, 65)");
  SAME(bad(65, off, {3, 99, 64, -5, 70}, 3), "seeds[1] = 99 is not a pod in [0, 65)");
  SAME(bad(64, off, good, 3), "seeds[2] = 64 is not a pod in [0, 64)");
  SAME(bad(1, {0, 1}, {0}, 1), "");
  SAME(bad(1, {0, 1}, {1}, 1), "seeds[0] = 1 is not a pod in [0, 1)");
  SAME(bad(0, {0, 1}, {0}, 1), "seeds[0] = 0 is not a pod in [0, 0)");
  // the working set: n_sets * max(W, 1) <= 2^24
  EXPECT(!reach_size_bad(1, REACH_WORDS_MAX));
  EXPECT(!reach_size_bad(0, REACH_WORDS_MAX));
  EXPECT(!reach_size_bad(1563, REACH_WORDS_MAX / 1563));
  EXPECT(!reach_size_bad(REACH_WORDS_MAX, 1));
  EXPECT(!reach_size_bad(1 << 20, 0));
  for (const char* m : {reach_size_bad(1, REACH_WORDS_MAX + 1), reach_size_bad(0, REACH_WORDS_MAX + 1),
                        reach_size_bad(1563, REACH_WORDS_MAX / 1563 + 1), reach_size_bad(REACH_WORDS_MAX, 2),
                        reach_size_bad(3, int64_t(1) << 62)}) {
    EXPECT(m != nullptr);
    if (m) SAME(std::string(m), "n_sets * words exceeds the limit of 16777216 (2^24)");
  }
}

// bitsets and first levels against a tally per (set, pod)
static void check_bits(int P, int n_sets, int max_seeds) {
  ctx = "bits P " + std::to_string(P) + " sets " + std::to_string(n_sets);
  const int W = (P + 63) / 64;
  std::vector<int64_t> off{0};
  std::vector<int32_t> seeds;
  std::vector<std::vector<char>> is_seed(size_t(n_sets), std::vector<char>(size_t(P), 0));
  for (int j = 0; j < n_sets; j++) {
    const int n = j % 3 == 1 ? 0 : int(rnd() % (max_seeds + 1));  // (every third set is empty)
    for (int i = 0; i < n; i++) {
      // duplicates, and the pods at the edges of the words
      const int32_t p = i % 4 == 3 && !seeds.empty() && off.back() < int64_t(seeds.size()) ? seeds.back()
                        : i % 4 == 2                                                        ? P - 1
                                                                                            : int32_t(rnd() % P);
      seeds.push_back(p), is_seed[size_t(j)][size_t(p)] = 1;
    }
    off.push_back(int64_t(seeds.size()));
  }
  SAME(bad(P, off, seeds, n_sets), "");
  std::vector<uint64_t> bits{123};
  std::vector<int64_t> levels{7, 7};
  reach_seed_bits(W, off.data(), seeds.data(), n_sets, bits, levels);
  SAME(bits.size(), size_t(n_sets) * W);
  SAME(levels.size(), size_t(n_sets));
  if (bits.size() != size_t(n_sets) * W || levels.size() != size_t(n_sets)) return;
  for (int j = 0; j < n_sets; j++) {
    bool any = false;
    for (int b = 0; b < W * 64; b++) {
      const bool got = (bits[size_t(j) * W + b / 64] >> (b % 64)) & 1;
      const bool want = b < P && is_seed[size_t(j)][size_t(b)];
      any = any || want;
      if (got != want) EXPECT(!"a bit of the seed bitsets differs from the tally");
    }
    SAME(levels[size_t(j)], any ? 0 : -1);
  }
}

// a search pod by pod over a random digraph: the counters per hop as the step delivers them -> levels
static void check_levels(int P, int n_sets) {
  ctx = "levels P " + std::to_string(P) + " sets " + std::to_string(n_sets);
  std::vector<char> edge(size_t(P) * P, 0);
  for (int i = 0; i < 2 * P; i++) edge[size_t(rnd() % P) * P + rnd() % P] = 1;
  std::vector<int64_t> off{0};
  std::vector<int32_t> seeds;
  for (int j = 0; j < n_sets; j++) {
    for (int i = 0, n = j % 4 == 2 ? 0 : 1 + int(rnd() % 3); i < n; i++) seeds.push_back(int32_t(rnd() % P));
    off.push_back(int64_t(seeds.size()));
  }
  std::vector<uint64_t> bits;
  std::vector<int64_t> levels;
  reach_seed_bits((P + 63) / 64, off.data(), seeds.data(), n_sets, bits, levels);
  std::vector<std::vector<int>> hop_of(size_t(n_sets), std::vector<int>(size_t(P), -1));
  for (int j = 0; j < n_sets; j++)
    for (int64_t i = off[size_t(j)]; i < off[size_t(j) + 1]; i++) hop_of[size_t(j)][size_t(seeds[size_t(i)])] = 0;
  int hops_run = 0;
  for (int hop = 1;; hop++) {
    std::vector<unsigned long long> cnt(size_t(n_sets), 0);
    for (int j = 0; j < n_sets; j++) {
      auto& h = hop_of[size_t(j)];
      for (int d = 0; d < P; d++) {
        if (h[size_t(d)] >= 0) continue;
        for (int s = 0; s < P; s++)
          if (h[size_t(s)] == hop - 1 && edge[size_t(s) * P + d]) {
            h[size_t(d)] = hop, cnt[size_t(j)]++;
            break;
          }
      }
    }
    hops_run = hop;
    if (!reach_levels(cnt.data(), n_sets, hop, levels.data())) break;
  }
  EXPECT(hops_run >= (P > 64 ? 2 : 1));
  for (int j = 0; j < n_sets; j++) {
    int want = -1;
    for (int p = 0; p < P; p++) want = hop_of[size_t(j)][size_t(p)] > want ? hop_of[size_t(j)][size_t(p)] : want;
    SAME(levels[size_t(j)], int64_t(want));
  }
}

int main() {
  check_refusals();
  for (int P : {1, 63, 64, 65, 128, 129, 1000})
    for (int n_sets : {0, 1, 3, 7}) check_bits(P, n_sets, P < 64 ? 5 : 40);
  for (int P : {1, 64, 65, 200})
    for (int n_sets : {1, 5}) check_levels(P, n_sets);
  if (failures) return std::printf("reach terms: %d failures\n", failures), 1;
  std::printf("reach terms: ok\n");
  return 0;
}
