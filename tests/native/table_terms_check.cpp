// table_terms_check.cpp — the host arithmetic of the device-table entry points (cyclonus_amd/csrc/table_terms.hpp)
// on the CPU.  For small random tables the counter arrays a kernel pass would deliver are built by a literal loop
// over the cells, from the layout comments of dev_table.hpp (TileArgs::cnt / src_cnt, GroupArgs::t.cnt,
// RowCountArgs::cnt; the compare's per-slot counters hold the cells where table a has a job, as the kernels' "per
// job" comments say), the terms functions run on them, and every output is compared with a per-cell tally of
// cyc_table_cells' code rule (jobrunner.go:36-55,85-93) and of comparisontable.go's rule as tests/test_comparison.py
// states it, both written out here.  GroupTables and find's paging are checked on their own.
// Built with g++ under ASan + UBSan and run by tests/test_table_terms.py; exits non-zero on a mismatch.
#include <cstdio>
#include <string>
#include <vector>

#include "table_terms.hpp"

using namespace cyc;
using Vec = std::vector<int64_t>;
using Cnt = std::vector<cnt_t>;

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

constexpr int64_t JUNK = -12345;  // outputs a function writes in full start as this

// One table's whole problem: the statuses and both planes' bits of every cell.
struct Planes {
  int P, K;
  std::vector<uint8_t> st, in, eg;  // st[d][k]; in[d][k][s]; eg[s][k][d]
  Planes(int P_, int K_, int first) : P(P_), K(K_), st(size_t(P_) * K_), in(size_t(P_) * K_ * P_), eg(in.size()) {
    for (auto& x : in) x = rnd() & 1;
    for (auto& x : eg) x = rnd() & 1;
    for (auto& x : st) x = rnd() % 3 ? uint8_t(rnd() & 3) : uint8_t(CYC_JOB_VALID);
    for (size_t i = 0; i < 4 && i < st.size(); i++) st[i] = uint8_t((first + i) & 3);  // all four values are there
  }
  // cyc_table_cells' code of cell (s, d, k) in a view
  int code(int view, int s, int d, int k) const {
    const uint8_t j = st[size_t(d) * K + k];
    if (j == CYC_JOB_NONE) return CYC_CONN_NO_JOB;
    if (j == CYC_JOB_VALID) {
      const bool i = in[(size_t(d) * K + k) * P + s], e = eg[(size_t(s) * K + k) * P + d];
      return (view == CYC_VIEW_INGRESS ? i : view == CYC_VIEW_EGRESS ? e : i && e) ? CYC_CONN_ALLOWED : CYC_CONN_BLOCKED;
    }
    if (view == CYC_VIEW_EGRESS) return CYC_CONN_UNKNOWN;
    return j == CYC_JOB_BAD_NAMED_PORT ? CYC_CONN_INVALID_NAMED_PORT : CYC_CONN_INVALID_PORT_PROTOCOL;
  }
  bool job(int d, int k) const { return st[size_t(d) * K + k] != CYC_JOB_NONE; }
};
// comparisontable.go: a job's results differ when the Combined codes do (a slot only one table has a job in
// differs); a pair differs when any slot does
static bool differs(const Planes& a, const Planes& b, int s, int d, int k) {
  return a.code(CYC_VIEW_COMBINED, s, d, k) != b.code(CYC_VIEW_COMBINED, s, d, k);
}
static bool pair_differs(const Planes& a, const Planes& b, int s, int d, int k_lo, int k_hi) {
  for (int k = k_lo; k < k_hi; k++)
    if (differs(a, b, s, d, k)) return true;
  return false;
}
// (same, different, ignored)
static int klass(bool differ, bool loopback_ignored) { return loopback_ignored ? 2 : differ ? 1 : 0; }

static TableShape shape(int P, int K, int lo, int hi, int part) {
  TableShape t;
  t.P = uint32_t(P), t.K = uint32_t(K), t.W = uint32_t((P + 63) / 64);
  t.row_lo = lo, t.row_hi = hi, t.partition = part;
  t.w0 = part == CYC_ROWS_SOURCE ? uint32_t(lo / 64) : 0;
  t.wa = part == CYC_ROWS_SOURCE ? uint32_t(hi > lo ? (hi + 63) / 64 - lo / 64 : 0) : t.W;
  return t;
}

static void check_counts_whole(const Planes& a, const TableShape& t, int k_lo, int k_hi) {
  const int P = a.P, nk = k_hi - k_lo;
  Cnt cnt(size_t(nk) * 3 * P, 0);  // TileArgs::cnt, counts: [nk][3][P]
  Vec want[3] = {Vec(nk * 6, 0), Vec(nk * 6, 0), Vec(nk * 6, 0)}, got[3] = {want[0], want[1], want[2]};
  int64_t want_nj = 0, got_nj = 0;
  for (int kk = 0; kk < nk; kk++)
    for (int v = 0; v < 3; v++)
      for (int d = 0; d < P; d++)
        for (int s = int(t.row_lo); s < t.row_hi; s++) {
          const int c = a.code(v, s, d, k_lo + kk);
          cnt[(size_t(kk) * 3 + v) * P + d] += c == CYC_CONN_ALLOWED;
          if (c != CYC_CONN_NO_JOB) want[v][kk * 6 + c]++;
          else if (v == CYC_VIEW_COMBINED) want_nj++;
        }
  int64_t* out[3] = {got[0].data(), got[1].data(), got[2].data()};
  counts_whole(t, a.st.data(), cnt.data(), k_lo, nk, out, &got_nj);
  for (int v = 0; v < 3; v++) SAME(got[v], want[v]);
  SAME(got_nj, want_nj);
  Vec eg_only(nk * 6, 0);  // one output alone
  int64_t* one[3] = {nullptr, eg_only.data(), nullptr};
  counts_whole(t, a.st.data(), cnt.data(), k_lo, nk, one, nullptr);
  SAME(eg_only, want[1]);
}

static void check_counts_partial(const Planes& a, const TableShape& t, int k_lo, int k_hi) {
  const int P = a.P, nk = k_hi - k_lo, rows = int(t.rows());
  Cnt cnt(size_t(rows) * nk * 2, 0);  // RowCountArgs::cnt: [rows][nk][2]
  Vec want_in(nk * 6, 0), want_eg(nk * 6, 0), got_in(nk * 6, 0), got_eg(nk * 6, 0);
  for (int r = 0; r < rows; r++)
    for (int kk = 0; kk < nk; kk++)
      for (int o = 0; o < P; o++) {  // the other end: a source of destination row r, a destination of source row r
        const int ci = a.code(CYC_VIEW_INGRESS, o, int(t.row_lo) + r, k_lo + kk), ce = a.code(CYC_VIEW_EGRESS, int(t.row_lo) + r, o, k_lo + kk);
        cnt[(size_t(r) * nk + kk) * 2] += ci == CYC_CONN_ALLOWED;
        cnt[(size_t(r) * nk + kk) * 2 + 1] += ce == CYC_CONN_ALLOWED;
        if (ci != CYC_CONN_NO_JOB) want_in[kk * 6 + ci]++;
        if (ce != CYC_CONN_NO_JOB) want_eg[kk * 6 + ce]++;
      }
  counts_partial(t, a.st.data(), cnt.data(), k_lo, nk, got_in.data(), got_eg.data());
  SAME(got_in, want_in);
  SAME(got_eg, want_eg);
  Vec in_only(nk * 6, 0);
  counts_partial(t, a.st.data(), cnt.data(), k_lo, nk, in_only.data(), nullptr);
  SAME(in_only, want_in);
}

static void check_pod_counts(const Planes& a, const TableShape& t, int view, int k_lo, int k_hi) {
  const int P = a.P, nk = k_hi - k_lo, rows = int(t.rows());
  const size_t stride = size_t(t.wa) * 64;
  Cnt cnt(size_t(nk) * 3 * P, 0), src(size_t(nk) * stride, 0);  // TileArgs::cnt and src_cnt ([nk][WA * 64]), counts
  Vec want_s(size_t(rows) * nk * 7, 0), want_d(size_t(P) * nk * 7, 0), got_s(want_s.size(), JUNK), got_d(want_d.size(), JUNK);
  for (int kk = 0; kk < nk; kk++)
    for (int d = 0; d < P; d++)
      for (int s = int(t.row_lo); s < t.row_hi; s++) {
        for (int v = 0; v < 3; v++) cnt[(size_t(kk) * 3 + v) * P + d] += a.code(v, s, d, k_lo + kk) == CYC_CONN_ALLOWED;
        const int c = a.code(view, s, d, k_lo + kk), col = c == CYC_CONN_NO_JOB ? 6 : c;
        src[kk * stride + size_t(s - 64 * int(t.w0))] += c == CYC_CONN_ALLOWED;
        want_s[(size_t(s - t.row_lo) * nk + kk) * 7 + col]++;
        want_d[(size_t(d) * nk + kk) * 7 + col]++;
      }
  pod_counts(t, a.st.data(), cnt.data(), src.data(), view, k_lo, nk, got_s.data(), got_d.data());
  SAME(got_s, want_s);
  SAME(got_d, want_d);
  Vec d_only(want_d.size(), JUNK);
  pod_counts(t, a.st.data(), cnt.data(), nullptr, view, k_lo, nk, nullptr, d_only.data());
  SAME(d_only, want_d);
}

static void check_compare(const Planes& a, const Planes& b, const TableShape& t, int k_lo, int k_hi, int il) {
  const int P = a.P, nk = k_hi - k_lo, rows = int(t.rows());
  const size_t stride = size_t(t.wa) * 64;
  Cnt cnt(size_t(nk + 2) * P, 0), src(size_t(nk + 1) * stride, 0);  // TileArgs::cnt [nk + 2][P], src_cnt [nk + 1][WA * 64], compare
  Vec w_pairs(3, 0), w_slots(nk * 3, 0), w_dst(size_t(P) * nk * 3, 0), w_sp(size_t(rows) * 3, 0), w_dp(size_t(P) * 3, 0),
      w_ss(size_t(rows) * nk * 3, 0);
  for (int d = 0; d < P; d++)
    for (int s = int(t.row_lo); s < t.row_hi; s++) {
      const bool loop = il && s == d, pd = pair_differs(a, b, s, d, k_lo, k_hi);
      const size_t i = size_t(s - t.row_lo);
      cnt[size_t(nk) * P + d] += pd, src[nk * stride + size_t(s - 64 * int(t.w0))] += pd;
      if (s == d) cnt[size_t(nk + 1) * P + d] = pd;
      w_pairs[klass(pd, loop)]++, w_sp[i * 3 + klass(pd, loop)]++, w_dp[size_t(d) * 3 + klass(pd, loop)]++;
      for (int kk = 0; kk < nk; kk++) {
        if (!a.job(d, k_lo + kk)) continue;
        const bool df = differs(a, b, s, d, k_lo + kk);
        cnt[size_t(kk) * P + d] += df && !loop, src[kk * stride + size_t(s - 64 * int(t.w0))] += df && !loop;
        w_slots[kk * 3 + klass(df, loop)]++, w_dst[(size_t(d) * nk + kk) * 3 + klass(df, loop)]++;
        w_ss[(i * nk + kk) * 3 + klass(df, loop)]++;
      }
    }
  Vec pairs(3, JUNK), slots(w_slots.size(), JUNK), dst(w_dst.size(), JUNK);
  compare_pairs(t, cnt.data(), nk, il, pairs.data());
  compare_jobs_by_dst(t, a.st.data(), cnt.data(), k_lo, nk, il, slots.data(), dst.data());
  SAME(pairs, w_pairs);
  SAME(slots, w_slots);
  SAME(dst, w_dst);
  Vec slots_only(w_slots.size(), JUNK);
  compare_jobs_by_dst(t, a.st.data(), cnt.data(), k_lo, nk, il, slots_only.data(), nullptr);
  SAME(slots_only, w_slots);
  Vec sp(w_sp.size(), JUNK), dp(w_dp.size(), JUNK), ss(w_ss.size(), JUNK), ds(w_dst.size(), JUNK);
  pod_compare(t, a.st.data(), cnt.data(), src.data(), k_lo, nk, il, sp.data(), dp.data(), ss.data(), ds.data());
  SAME(sp, w_sp);
  SAME(dp, w_dp);
  SAME(ss, w_ss);
  SAME(ds, w_dst);
  Vec dp_only(w_dp.size(), JUNK);
  pod_compare(t, a.st.data(), cnt.data(), nullptr, k_lo, nk, il, nullptr, dp_only.data(), nullptr, nullptr);
  SAME(dp_only, w_dp);
}

// ---- groupings
static std::vector<int32_t> grouping(int P, int kind, int64_t* G) {
  std::vector<int32_t> g(size_t(P), 0);
  if (kind == 0) return *G = 1, g;  // every pod in the one group
  if (kind == 3) {  // group 1 straddles the word boundary at pod 64, group 2 has no pod, some pods have none
    for (int p = 0; p < P; p++) g[size_t(p)] = p >= 60 && p < 70 ? 1 : p % 5 == 4 ? -1 : 0;
    return *G = 3, g;
  }
  *G = kind == 1 ? 3 : 40;  // 40: more than GT_CAP groups in one block
  for (auto& x : g) x = int32_t(rnd() % uint32_t(*G + 1)) - 1;
  return g;
}

static void check_group_tables(const TableShape& t, const std::vector<int32_t>& g, int64_t G) {
  const GroupTables gt(t, g.data(), G);
  Vec n_src(size_t(G), 0), n_dst(size_t(G), 0);
  for (int64_t p = 0; p < int64_t(t.P); p++)
    if (g[size_t(p)] >= 0) n_dst[size_t(g[size_t(p)])]++, n_src[size_t(g[size_t(p)])] += t.has_row(p);
  SAME(gt.n_src, n_src);
  SAME(gt.n_dst, n_dst);
  SAME(gt.ent_ptr.size(), size_t(t.wa) + 1);
  SAME(gt.row_ptr.size(), size_t(t.wa + GROUP_TILE_WORDS - 1) / GROUP_TILE_WORDS + 1);
  EXPECT(gt.ent_grp.size() == gt.ent_mask.size() && gt.ent_loc.size() == gt.ent_mask.size() && gt.ent_ptr.back() == gt.ent_mask.size());
  for (uint32_t j = 0; j < t.wa; j++) {
    uint64_t seen = 0, want = 0;
    int last_first = -1;
    for (int bit = 0; bit < 64; bit++) {
      const int64_t s = int64_t(t.w0 + j) * 64 + bit;
      if (t.has_row(s) && g[size_t(s)] >= 0) want |= 1ull << bit;
    }
    EXPECT(gt.ent_ptr[j] <= gt.ent_ptr[j + 1]);
    for (uint32_t e = gt.ent_ptr[j]; e < gt.ent_ptr[j + 1]; e++) {
      const uint64_t m = gt.ent_mask[e];
      EXPECT(m != 0 && (m & seen) == 0);  // disjoint
      seen |= m;
      const int first = __builtin_ctzll(m | 1ull << 63);
      EXPECT(first > last_first);  // pod order
      last_first = first;
      for (int bit = 0; bit < 64; bit++)
        if (m >> bit & 1) EXPECT((want >> bit & 1) && uint32_t(g[size_t(t.w0 + j) * 64 + size_t(bit)]) == gt.ent_grp[e]);
      const uint32_t r = j / GROUP_TILE_WORDS;  // the entry's block row resolves its local number to its group
      EXPECT(gt.row_ptr[r] + gt.ent_loc[e] < gt.row_ptr[r + 1] && gt.row_grp[gt.row_ptr[r] + gt.ent_loc[e]] == gt.ent_grp[e]);
    }
    SAME(seen, want);  // cover exactly the grouped pods of the table's rows
  }
  SAME(gt.col_ptr.size(), size_t(t.P + GROUP_TILE_WORDS * 64 - 1) / (GROUP_TILE_WORDS * 64) + 1);
  SAME(gt.dst_loc.size(), size_t(t.P));
  for (uint32_t d = 0; d < t.P; d++) {
    if (g[d] < 0) continue;
    const uint32_t c = d / (GROUP_TILE_WORDS * 64);
    EXPECT(gt.col_ptr[c] + gt.dst_loc[d] < gt.col_ptr[c + 1] && gt.col_grp[gt.col_ptr[c] + gt.dst_loc[d]] == uint32_t(g[d]));
  }
  for (size_t r = 0; r + 1 < gt.row_ptr.size(); r++)  // a group is numbered once per block row and column
    for (uint32_t x = gt.row_ptr[r]; x < gt.row_ptr[r + 1]; x++)
      for (uint32_t y = x + 1; y < gt.row_ptr[r + 1]; y++) EXPECT(gt.row_grp[x] != gt.row_grp[y]);
  for (size_t c = 0; c + 1 < gt.col_ptr.size(); c++)
    for (uint32_t x = gt.col_ptr[c]; x < gt.col_ptr[c + 1]; x++)
      for (uint32_t y = x + 1; y < gt.col_ptr[c + 1]; y++) EXPECT(gt.col_grp[x] != gt.col_grp[y]);
}

static void check_groups(const Planes& a, const Planes& b, const TableShape& t, const std::vector<int32_t>& g, int64_t G, int k_lo,
                         int k_hi) {
  const int P = a.P, nk = k_hi - k_lo;
  const size_t GG = size_t(G * G);
  const GroupTables gt(t, g.data(), G);
  {
    Cnt cnt(size_t(nk) * 3 * GG, 0);  // GroupArgs::t.cnt, counts: [nk][3][G][G]
    Vec want[3] = {Vec(GG * nk * 6, 0), Vec(GG * nk * 6, 0), Vec(GG * nk * 6, 0)}, got[3] = {want[0], want[1], want[2]};
    Vec want_nj(GG, 0), got_nj(GG, 0);
    for (int d = 0; d < P; d++)
      for (int s = int(t.row_lo); s < t.row_hi; s++) {
        if (g[size_t(s)] < 0 || g[size_t(d)] < 0) continue;
        const size_t pair = size_t(g[size_t(s)]) * size_t(G) + size_t(g[size_t(d)]);
        for (int kk = 0; kk < nk; kk++)
          for (int v = 0; v < 3; v++) {
            const int c = a.code(v, s, d, k_lo + kk);
            cnt[(size_t(kk) * 3 + v) * GG + pair] += c == CYC_CONN_ALLOWED;
            if (c != CYC_CONN_NO_JOB) want[v][(pair * nk + kk) * 6 + c]++;
            else if (v == CYC_VIEW_COMBINED) want_nj[pair]++;
          }
      }
    int64_t* out[3] = {got[0].data(), got[1].data(), got[2].data()};
    group_counts(t, a.st.data(), cnt.data(), g.data(), gt, k_lo, nk, out, got_nj.data());
    for (int v = 0; v < 3; v++) SAME(got[v], want[v]);
    SAME(got_nj, want_nj);
  }
  for (int il = 0; il < 2; il++) {
    Cnt cnt(size_t(nk + 1) * GG + size_t(G), 0);  // GroupArgs::t.cnt, compare: [nk + 1][G][G], then [G]
    Vec w_pairs(GG * 3, 0), w_slots(GG * nk * 3, 0), pairs(GG * 3, 0), slots(GG * nk * 3, 0);
    for (int d = 0; d < P; d++)
      for (int s = int(t.row_lo); s < t.row_hi; s++) {
        if (g[size_t(s)] < 0 || g[size_t(d)] < 0) continue;
        const size_t pair = size_t(g[size_t(s)]) * size_t(G) + size_t(g[size_t(d)]);
        const bool loop = il && s == d, pd = pair_differs(a, b, s, d, k_lo, k_hi);
        cnt[size_t(nk) * GG + pair] += pd;
        if (s == d) cnt[size_t(nk + 1) * GG + size_t(g[size_t(d)])] += pd;
        w_pairs[pair * 3 + klass(pd, loop)]++;
        for (int kk = 0; kk < nk; kk++) {
          if (!a.job(d, k_lo + kk)) continue;
          const bool df = differs(a, b, s, d, k_lo + kk);
          cnt[size_t(kk) * GG + pair] += df && !loop;
          w_slots[(pair * nk + kk) * 3 + klass(df, loop)]++;
        }
      }
    group_compare(t, a.st.data(), cnt.data(), g.data(), gt, k_lo, nk, il, pairs.data(), slots.data());
    SAME(pairs, w_pairs);
    SAME(slots, w_slots);
    Vec pairs_only(GG * 3, 0);
    group_compare(t, a.st.data(), cnt.data(), g.data(), gt, k_lo, nk, il, pairs_only.data(), nullptr);
    SAME(pairs_only, w_pairs);
  }
}

static void check_shape(int P, int K, int lo, int hi, int part, int first) {
  const Planes a(P, K, first), b(P, K, first + 1);
  const TableShape t = shape(P, K, lo, hi, part);
  std::vector<std::vector<int32_t>> gs;
  std::vector<int64_t> Gs;
  for (int kind = 0; kind < 4 && t.whole(); kind++) {
    int64_t G;
    gs.push_back(grouping(P, kind, &G)), Gs.push_back(G);
    ctx = "P " + std::to_string(P) + " rows [" + std::to_string(lo) + ", " + std::to_string(hi) + ") grouping " + std::to_string(kind);
    check_group_tables(t, gs.back(), G);
  }
  for (int k_lo = 0; k_lo <= K; k_lo++)
    for (int k_hi = k_lo; k_hi <= K; k_hi++) {  // every slot sub-range, the empty ones too
      ctx = "P " + std::to_string(P) + " K " + std::to_string(K) + " rows [" + std::to_string(lo) + ", " + std::to_string(hi) + ") partition " +
            std::to_string(part) + " slots [" + std::to_string(k_lo) + ", " + std::to_string(k_hi) + ")";
      if (!t.whole()) {
        check_counts_partial(a, t, k_lo, k_hi);
        continue;
      }
      check_counts_whole(a, t, k_lo, k_hi);
      for (int v = 0; v < 3; v++) check_pod_counts(a, t, v, k_lo, k_hi);
      for (int il = 0; il < 2; il++) check_compare(a, b, t, k_lo, k_hi, il);
      for (size_t i = 0; i < gs.size(); i++) check_groups(a, b, t, gs[i], Gs[i], k_lo, k_hi);
    }
}

// The status rule itself, and what it does with a value outside cyc_job_status
static void check_status_rule() {
  ctx = "status rule";
  for (int v = 0; v < 3; v++) {
    SAME(status_code(v, CYC_JOB_NONE), int(CYC_CONN_NO_JOB));
    SAME(status_code(v, CYC_JOB_BAD_NAMED_PORT), v == CYC_VIEW_EGRESS ? int(CYC_CONN_UNKNOWN) : int(CYC_CONN_INVALID_NAMED_PORT));
    SAME(status_code(v, CYC_JOB_BAD_PORT_PROTOCOL), v == CYC_VIEW_EGRESS ? int(CYC_CONN_UNKNOWN) : int(CYC_CONN_INVALID_PORT_PROTOCOL));
    for (int s : {4, 7, 200, 255}) SAME(status_code(v, uint8_t(s)), status_code(v, CYC_JOB_BAD_NAMED_PORT));
  }
  for (int s = 0; s < 256; s++) SAME(int(status_norm(uint8_t(s))), s < 4 ? s : int(CYC_JOB_BAD_NAMED_PORT));
}

static void check_paging() {
  const Cnt c = {3, 0, 5, 0, 0, 2};  // matches of sources 10..15; prefix sums 3 3 8 8 8 10
  int64_t total, n, s_next;
  Cnt offs;
  std::string why;
  auto page = [&](const cnt_t* cp, int64_t rows, int64_t cap, bool count_only) {
    why.clear();
    return find_page(cp, rows, 10, cap, count_only, &total, &n, &s_next, offs, why);
  };
  ctx = "paging: cap at a prefix's exact size";
  EXPECT(page(c.data(), 6, 8, false) && total == 10 && n == 8 && s_next == 15 && offs == Cnt({0, 3, 3, 8, 8, 8}));
  ctx = "paging: cap one below it (the sources without matches before it still belong to the page)";
  EXPECT(page(c.data(), 6, 7, false) && total == 10 && n == 3 && s_next == 12 && offs == Cnt({0, 3, 3}));
  ctx = "paging: cap holds everything";
  EXPECT(page(c.data(), 6, 10, false) && n == 10 && s_next == 16 && offs == Cnt({0, 3, 3, 8, 8, 8, 10}));
  EXPECT(page(c.data(), 6, 9, false) && n == 8 && s_next == 15);
  ctx = "paging: cap below the first source's count";
  EXPECT(!page(c.data(), 6, 2, false) && total == 10 && n == 0 && s_next == 10);
  SAME(why, std::string("source 10 alone has 3 matching cells, more than cap 2"));
  EXPECT(!page(c.data(), 6, 0, false) && why == "source 10 alone has 3 matching cells, more than cap 0");
  ctx = "paging: sources without matches";
  EXPECT(page(c.data() + 3, 2, 0, false) && total == 0 && n == 0 && s_next == 12 && offs == Cnt({0, 0, 0}));
  EXPECT(page(c.data() + 1, 1, 0, false) && n == 0 && s_next == 11);
  ctx = "paging: count only";
  EXPECT(page(c.data(), 6, 0, true) && total == 10 && n == 0 && s_next == 10);
  EXPECT(page(c.data(), 6, 100, true) && total == 10 && n == 0 && s_next == 10);
  ctx = "paging: no slot (nk == 0) or no source";
  EXPECT(page(nullptr, 6, 4, false) && total == 0 && n == 0 && s_next == 16);
  EXPECT(page(nullptr, 6, 0, true) && total == 0 && n == 0 && s_next == 10);
  EXPECT(page(nullptr, 0, 4, false) && total == 0 && n == 0 && s_next == 10);
}

static void check_group_args() {
  ctx = "group_args_bad";
  const TableShape t = shape(5, 3, 0, 5, CYC_ROWS_TARGET);
  const int32_t g[5] = {0, -1, 2, 1, 0};
  std::string why;
  EXPECT(group_args_bad(t, g, 3, 0, 3, why) == nullptr && group_args_bad(t, g, 3, 2, 2, why) == nullptr);
  SAME(std::string(group_args_bad(t, nullptr, 3, 0, 3, why)), std::string("null group_of"));
  SAME(std::string(group_args_bad(t, g, 3, 0, 4, why)), std::string("slot range out of bounds"));
  SAME(std::string(group_args_bad(t, g, 3, -1, 2, why)), std::string("slot range out of bounds"));
  SAME(std::string(group_args_bad(t, g, 3, 2, 1, why)), std::string("slot range out of bounds"));
  SAME(std::string(group_args_bad(t, g, 0, 0, 3, why)), std::string("n_groups must be at least 1"));
  SAME(std::string(group_args_bad(t, g, 11586, 0, 1, why)), std::string("n_groups^2 * slots exceeds the limit of 134217728 (2^27)"));
  SAME(std::string(group_args_bad(t, g, int64_t(1) << 40, 0, 1, why)), std::string("n_groups^2 * slots exceeds the limit of 134217728 (2^27)"));
  SAME(std::string(group_args_bad(t, g, 2, 0, 3, why)), std::string("group_of[2] = 2 is neither -1 nor a group in [0, 2)"));
  const int32_t low[5] = {0, -2, 0, 0, 0};
  SAME(std::string(group_args_bad(t, low, 2, 0, 3, why)), std::string("group_of[1] = -2 is neither -1 nor a group in [0, 2)"));
}

int main() {
  check_status_rule();
  check_paging();
  check_group_args();
  int first = 0;
  for (int P : {1, 63, 64, 65, 130})
    for (int K : {1, 3}) {
      check_shape(P, K, 0, P, CYC_ROWS_TARGET, first++);
      if (P != 130) continue;
      check_shape(P, K, 0, 64, CYC_ROWS_SOURCE, first++);
      check_shape(P, K, 64, 130, CYC_ROWS_SOURCE, first++);
      check_shape(P, K, 10, 70, CYC_ROWS_TARGET, first++);  // partial target rows: counts of Ingress and Egress only
    }
  // GroupTables past one block row of 16 source words and one block column of 1024 destinations
  for (int kind = 0; kind < 4; kind++) {
    int64_t G;
    const std::vector<int32_t> g = grouping(2100, kind, &G);
    ctx = "P 2100 grouping " + std::to_string(kind);
    check_group_tables(shape(2100, 1, 0, 2100, CYC_ROWS_TARGET), g, G);
    check_group_tables(shape(2100, 1, 1024, 2100, CYC_ROWS_SOURCE), g, G);
  }
  if (failures) return std::printf("table terms: %d failures\n", failures), 1;
  std::printf("table terms: ok\n");
  return 0;
}
