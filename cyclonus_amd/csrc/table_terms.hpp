// table_terms.hpp — the host arithmetic of the device-table entry points (table.hpp): from the counters a kernel pass
// delivers, in exactly the layouts dev_table.hpp documents, and table a's status plane to the documented outputs of
// include/cyclonus_hip.h.  Plain integer C++ without HIP (tests/native/table_terms_check.cpp runs it on the CPU).
#pragma once

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "cyclonus_hip.h"

namespace cyc {

using cnt_t = unsigned long long;  // a device counter

struct TableShape {  // (the terms take it by value: the loops' stores to the outputs cannot alias a local copy)
  uint32_t P = 0, K = 0, W = 0;
  int64_t row_lo = 0, row_hi = 0;
  int partition = CYC_ROWS_TARGET;  // CYC_ROWS_SOURCE: rows are sources; ingress rows cover words [w0, w0 + wa)
  uint32_t w0 = 0, wa = 0;
  int64_t rows() const { return row_hi - row_lo; }
  // every cell (s in the rows, d, k) has both directions: a source-row table, or all target rows
  bool whole() const { return partition == CYC_ROWS_SOURCE || (row_lo == 0 && row_hi == int64_t(P)); }
  bool has_row(int64_t p) const { return p >= row_lo && p < row_hi; }
};

// cyc_table_cells' code (jobrunner.go:36-55) of a cell in `view` whose job's status is not VALID: CYC_CONN_NO_JOB
// where there is no job; otherwise Egress is unknown, Ingress and Combined name the bad port.  A status outside
// cyc_job_status is outside the contract of include/cyclonus_hip.h; the host counts it as BAD_NAMED_PORT.
inline uint8_t status_norm(uint8_t s) { return s <= CYC_JOB_BAD_PORT_PROTOCOL ? s : uint8_t(CYC_JOB_BAD_NAMED_PORT); }
inline int status_code(int view, uint8_t s) {
  if (s == CYC_JOB_NONE) return CYC_CONN_NO_JOB;
  if (view == CYC_VIEW_EGRESS) return CYC_CONN_UNKNOWN;
  return s == CYC_JOB_BAD_PORT_PROTOCOL ? CYC_CONN_INVALID_PORT_PROTOCOL : CYC_CONN_INVALID_NAMED_PORT;
}

// cyc_table_counts of a whole table.  cnt: TileArgs::cnt of the counts, [nk][3][P].  out[view]: [nk][6] or null.
// All outputs arrive zeroed.
inline void counts_whole(const TableShape t, const uint8_t* st, const cnt_t* cnt, int64_t k_lo, int64_t nk, int64_t* const out[3],
                         int64_t* no_job) {
  const int64_t P = t.P, rows = t.rows();
  for (int64_t kk = 0; kk < nk; kk++)
    for (int64_t d = 0; d < P; d++) {
      const uint8_t s = st[d * t.K + k_lo + kk];
      if (s == CYC_JOB_NONE && no_job) *no_job += rows;
      for (int x = 0; x < 3; x++) {
        if (!out[x] || s == CYC_JOB_NONE) continue;
        int64_t* o = out[x] + kk * 6;
        if (s == CYC_JOB_VALID) {
          const int64_t a = int64_t(cnt[(kk * 3 + x) * P + d]);
          o[CYC_CONN_ALLOWED] += a, o[CYC_CONN_BLOCKED] += rows - a;
        } else {
          o[status_code(x, s)] += rows;
        }
      }
    }
}

// cyc_table_counts of a partial target-row table: Ingress over (every source, the rows' destinations), Egress over
// (the rows' sources, every destination).  cnt: RowCountArgs::cnt, [rows][nk][2].
inline void counts_partial(const TableShape t, const uint8_t* st, const cnt_t* cnt, int64_t k_lo, int64_t nk, int64_t* ingress,
                           int64_t* egress) {
  const int64_t P = t.P, rows = t.rows();
  for (int64_t kk = 0; kk < nk; kk++) {
    int64_t* oi = ingress ? ingress + kk * 6 : nullptr;
    int64_t* oe = egress ? egress + kk * 6 : nullptr;
    for (int64_t d = 0; d < P; d++) {
      const uint8_t s = st[d * t.K + k_lo + kk];
      if (s == CYC_JOB_NONE) continue;
      if (s == CYC_JOB_VALID) {
        if (oi && t.has_row(d)) {
          const int64_t a = int64_t(cnt[((d - t.row_lo) * nk + kk) * 2]);
          oi[CYC_CONN_ALLOWED] += a, oi[CYC_CONN_BLOCKED] += P - a;
        }
        if (oe) oe[CYC_CONN_BLOCKED] += rows;  // (the allowed ones move over below)
      } else {
        if (oi && t.has_row(d)) oi[status_code(CYC_VIEW_INGRESS, s)] += P;
        if (oe) oe[status_code(CYC_VIEW_EGRESS, s)] += rows;
      }
    }
    for (int64_t r = 0; oe && r < rows; r++) {
      const int64_t a = int64_t(cnt[(r * nk + kk) * 2 + 1]);
      oe[CYC_CONN_ALLOWED] += a, oe[CYC_CONN_BLOCKED] -= a;
    }
  }
}

// cyc_table_pod_counts.  cnt: TileArgs::cnt of the counts; src: TileArgs::src_cnt, [nk][wa * 64] of `view` (read
// only with by_src).  The code of a destination's slot that is not VALID holds for every source, so a source's row
// has as many cells of it as there are such destinations.
inline void pod_counts(const TableShape t, const uint8_t* st, const cnt_t* cnt, const cnt_t* src, int view, int64_t k_lo, int64_t nk,
                       int64_t* by_src, int64_t* by_dst) {
  const int64_t P = t.P, rows = t.rows(), src_stride = int64_t(t.wa) * 64;
  int col[4];  // the output column of a status that is not VALID
  for (int s = 0; s < 4; s++) col[s] = s == CYC_JOB_NONE ? CYC_POD_CODES - 1 : status_code(view, uint8_t(s));
  for (int64_t kk = 0; kk < nk; kk++) {
    int64_t n_of[4] = {0, 0, 0, 0};  // destinations per cyc_job_status
    for (int64_t d = 0; d < P; d++) {
      const uint8_t s = status_norm(st[d * t.K + k_lo + kk]);
      n_of[s]++;
      if (!by_dst) continue;
      int64_t* o = by_dst + (d * nk + kk) * CYC_POD_CODES;
      std::fill(o, o + CYC_POD_CODES, int64_t(0));
      if (s == CYC_JOB_VALID) {
        const int64_t a = int64_t(cnt[(kk * 3 + view) * P + d]);
        o[CYC_CONN_ALLOWED] = a, o[CYC_CONN_BLOCKED] = rows - a;
      } else {
        o[col[s]] = rows;
      }
    }
    for (int64_t i = 0; by_src && i < rows; i++) {
      int64_t* o = by_src + (i * nk + kk) * CYC_POD_CODES;
      std::fill(o, o + CYC_POD_CODES, int64_t(0));
      const int64_t a = int64_t(src[kk * src_stride + i]);
      o[CYC_CONN_ALLOWED] = a, o[CYC_CONN_BLOCKED] = n_of[CYC_JOB_VALID] - a;
      for (int s : {CYC_JOB_NONE, CYC_JOB_BAD_NAMED_PORT, CYC_JOB_BAD_PORT_PROTOCOL}) o[col[s]] += n_of[s];
    }
  }
}

// ---- the compare.  cnt: TileArgs::cnt of the compare, [nk + 2][P]; src: its src_cnt, [nk + 1][wa * 64].  il: 1 when
// loopback is ignored, else 0.  Triples are (same, different, ignored).

// ValueCounts (comparisontable.go:109-123): a pair is the Items' equalsDict (:26-36) unless it is an ignored
// loopback; the table answers the pairs (s in its rows, every d).
inline void compare_pairs(const TableShape t, const cnt_t* cnt, int64_t nk, int64_t il, int64_t pair_counts[3]) {
  const int64_t P = t.P;
  int64_t differ = 0, self_differ = 0;
  for (int64_t d = 0; d < P; d++) differ += int64_t(cnt[nk * P + d]), self_differ += int64_t(cnt[(nk + 1) * P + d]);
  pair_counts[2] = il * t.rows();
  pair_counts[1] = differ - il * self_differ;
  pair_counts[0] = t.rows() * P - pair_counts[1] - pair_counts[2];
}

// per job (ValueCountsByProtocol :89-107, ResultsByProtocol :14-20,69-79): every cell whose job a holds, summed
// (slot_counts [nk][3]) and per destination (dst_counts [P][nk][3]), each optional
inline void compare_jobs_by_dst(const TableShape t, const uint8_t* st, const cnt_t* cnt, int64_t k_lo, int64_t nk, int64_t il,
                                int64_t* slot_counts, int64_t* dst_counts) {
  const int64_t P = t.P;
  if (slot_counts) std::fill(slot_counts, slot_counts + nk * 3, int64_t(0));
  if (slot_counts || dst_counts)
    for (int64_t d = 0; d < P; d++)
      for (int64_t kk = 0; kk < nk; kk++) {
        int64_t v[3] = {0, 0, 0};
        if (st[d * t.K + k_lo + kk] != CYC_JOB_NONE) {
          v[2] = il && t.has_row(d) ? 1 : 0;
          v[1] = int64_t(cnt[kk * P + d]);
          v[0] = t.rows() - v[1] - v[2];
        }
        for (int x = 0; x < 3; x++) {
          if (slot_counts) slot_counts[kk * 3 + x] += v[x];
          if (dst_counts) dst_counts[(d * nk + kk) * 3 + x] = v[x];
        }
      }
}

// cyc_table_pod_compare: the pairs of destination d over the table's sources and of source s over every destination
// (the loopback pair is ignored whether it differs or not), and the jobs likewise.  Each output optional.
inline void pod_compare(const TableShape t, const uint8_t* st, const cnt_t* cnt, const cnt_t* src, int64_t k_lo, int64_t nk, int64_t il,
                        int64_t* src_pairs, int64_t* dst_pairs, int64_t* src_slots, int64_t* dst_slots) {
  const int64_t P = t.P, rows = t.rows(), src_stride = int64_t(t.wa) * 64;
  const cnt_t* self = cnt + (nk + 1) * P;  // whether the pair (d, d) differs
  for (int64_t d = 0; dst_pairs && d < P; d++) {
    int64_t* o = dst_pairs + d * 3;
    o[2] = il && t.has_row(d) ? 1 : 0;
    o[1] = int64_t(cnt[nk * P + d]) - il * int64_t(self[d]);
    o[0] = rows - o[1] - o[2];
  }
  for (int64_t i = 0; src_pairs && i < rows; i++) {
    int64_t* o = src_pairs + i * 3;
    o[2] = il;
    o[1] = int64_t(src[nk * src_stride + i]) - il * int64_t(self[t.row_lo + i]);
    o[0] = P - o[1] - o[2];
  }
  compare_jobs_by_dst(t, st, cnt, k_lo, nk, il, nullptr, dst_slots);
  // per job and source: a's jobs of slot kk are the destinations whose status is not NONE, the loopback cell is
  // ignored when (s, kk) is a job of a
  for (int64_t kk = 0; src_slots && kk < nk; kk++) {
    int64_t jobs = 0;
    for (int64_t d = 0; d < P; d++) jobs += st[d * t.K + k_lo + kk] != CYC_JOB_NONE;
    for (int64_t i = 0; i < rows; i++) {
      int64_t* o = src_slots + (i * nk + kk) * 3;
      o[2] = il && st[(t.row_lo + i) * t.K + k_lo + kk] != CYC_JOB_NONE ? 1 : 0;
      o[1] = int64_t(src[kk * src_stride + i]);
      o[0] = jobs - o[1] - o[2];
    }
  }
}

// ---- counts and comparison per pod-group pair
constexpr int64_t GROUP_CELLS_MAX = int64_t(1) << 27;  // n_groups^2 * slots of one call
constexpr uint32_t GROUP_TILE_WORDS = 16;              // k_table_group_tiles' block: TT_WORDS of dev_table.hpp

// The checks the two group entry points share; nullptr when the arguments are fine (`why` holds a built message).
inline const char* group_args_bad(const TableShape t, const int32_t* group_of, int64_t G, int64_t k_lo, int64_t k_hi, std::string& why) {
  if (!group_of) return "null group_of";
  if (k_lo < 0 || k_hi > int64_t(t.K) || k_lo > k_hi) return "slot range out of bounds";
  if (G < 1) return "n_groups must be at least 1";
  if (G > GROUP_CELLS_MAX || G * G * std::max<int64_t>(k_hi - k_lo, 1) > GROUP_CELLS_MAX)
    return "n_groups^2 * slots exceeds the limit of 134217728 (2^27)";
  for (int64_t p = 0; p < int64_t(t.P); p++)
    if (group_of[p] < -1 || group_of[p] >= G) {
      why = "group_of[" + std::to_string(p) + "] = " + std::to_string(group_of[p]) + " is neither -1 nor a group in [0, " + std::to_string(G) + ")";
      return why.c_str();
    }
  return nullptr;
}

// What k_table_group_tiles takes of a grouping (GroupArgs, dev_table.hpp), from one walk over the pods: the
// (group, mask) entries of every source word of the table in pod order, the groups of every block row of 16
// source words and block column of 1024 destinations numbered in order of appearance, and the group sizes
// for the host-side terms.
struct GroupTables {
  std::vector<uint32_t> ent_ptr{0}, ent_grp, ent_loc, row_ptr, row_grp, dst_loc, col_ptr, col_grp;
  std::vector<uint64_t> ent_mask;
  std::vector<int64_t> n_src, n_dst;  // pods of a group among the table's sources, among all destinations

  GroupTables(const TableShape t, const int32_t* group_of, int64_t G) : n_src(size_t(G), 0), n_dst(size_t(G), 0) {
    constexpr uint32_t NONE = ~0u, TW = GROUP_TILE_WORDS;
    const size_t n = size_t(G);
    std::vector<uint32_t> word_of(n, NONE), ent_of(n), blk_of(n, NONE), loc_of(n);
    for (uint32_t j = 0; j < t.wa; j++) {
      if (j % TW == 0) row_ptr.push_back(uint32_t(row_grp.size()));
      for (uint32_t b = 0; b < 64; b++) {
        const int64_t s = int64_t(t.w0 + j) * 64 + b;
        if (!t.has_row(s) || group_of[s] < 0) continue;
        const uint32_t g = uint32_t(group_of[s]);
        n_src[g]++;
        if (word_of[g] != j) {
          if (blk_of[g] != j / TW) {
            blk_of[g] = j / TW, loc_of[g] = uint32_t(row_grp.size()) - row_ptr.back();
            row_grp.push_back(g);
          }
          word_of[g] = j, ent_of[g] = uint32_t(ent_grp.size());
          ent_grp.push_back(g), ent_loc.push_back(loc_of[g]), ent_mask.push_back(0);
        }
        ent_mask[ent_of[g]] |= 1ull << b;
      }
      ent_ptr.push_back(uint32_t(ent_grp.size()));
    }
    row_ptr.push_back(uint32_t(row_grp.size()));
    std::fill(blk_of.begin(), blk_of.end(), NONE);
    dst_loc.assign(t.P, 0);
    for (uint32_t d = 0; d < t.P; d++) {
      if (d % (TW * 64) == 0) col_ptr.push_back(uint32_t(col_grp.size()));
      if (group_of[d] < 0) continue;
      const uint32_t g = uint32_t(group_of[d]);
      n_dst[g]++;
      if (blk_of[g] != d / (TW * 64)) {
        blk_of[g] = d / (TW * 64), loc_of[g] = uint32_t(col_grp.size()) - col_ptr.back();
        col_grp.push_back(g);
      }
      dst_loc[d] = loc_of[g];
    }
    col_ptr.push_back(uint32_t(col_grp.size()));
  }
};

// cyc_table_group_counts.  cnt: GroupArgs::t.cnt of the counts, [nk][3][G][G].  out[view]: [G][G][nk][6] or null,
// no_job [G][G]; all arrive zeroed.  Per (destination group, slot) the destinations of each status, times the
// sources of the source group.
inline void group_counts(const TableShape t, const uint8_t* st, const cnt_t* cnt, const int32_t* group_of, const GroupTables& gt,
                         int64_t k_lo, int64_t nk, int64_t* const out[3], int64_t* no_job) {
  const int64_t P = t.P, G = int64_t(gt.n_src.size()), GG = G * G;
  std::vector<int64_t> by_status(size_t(G * nk * 4), 0);  // [gd][kk][cyc_job_status]
  for (int64_t d = 0; d < P; d++)
    if (group_of[d] >= 0)
      for (int64_t kk = 0; kk < nk; kk++) by_status[size_t((group_of[d] * nk + kk) * 4 + status_norm(st[d * t.K + k_lo + kk]))]++;
  for (int64_t gs = 0; gs < G; gs++) {
    const int64_t ns = gt.n_src[size_t(gs)];
    if (!ns) continue;
    for (int64_t gd = 0; gd < G; gd++) {
      if (!gt.n_dst[size_t(gd)]) continue;
      for (int64_t kk = 0; kk < nk; kk++) {
        const int64_t* n_of = &by_status[size_t((gd * nk + kk) * 4)];
        for (int x = 0; x < 3; x++) {
          if (!out[x]) continue;
          const int64_t allowed = int64_t(cnt[(kk * 3 + x) * GG + gs * G + gd]);
          int64_t* o = out[x] + ((gs * G + gd) * nk + kk) * 6;
          o[CYC_CONN_ALLOWED] = allowed, o[CYC_CONN_BLOCKED] = ns * n_of[CYC_JOB_VALID] - allowed;
          for (int s : {CYC_JOB_BAD_NAMED_PORT, CYC_JOB_BAD_PORT_PROTOCOL}) o[status_code(x, uint8_t(s))] += ns * n_of[s];
        }
        if (no_job) no_job[gs * G + gd] += ns * n_of[CYC_JOB_NONE];
      }
    }
  }
}

// cyc_table_group_compare: the terms of compare_pairs and compare_jobs_by_dst per group pair.  cnt: GroupArgs::t.cnt
// of the compare, [nk + 1][G][G] then [G].  pair_counts [G][G][3], slot_counts [G][G][nk][3] (optional); zeroed.
inline void group_compare(const TableShape t, const uint8_t* st, const cnt_t* cnt, const int32_t* group_of, const GroupTables& gt,
                          int64_t k_lo, int64_t nk, int64_t il, int64_t* pair_counts, int64_t* slot_counts) {
  const int64_t P = t.P, G = int64_t(gt.n_src.size()), GG = G * G;
  // jobs[gd][kk] = destinations of the group where a holds a job, loop[g][kk] = those among the table's sources (the
  // loopback cells)
  std::vector<int64_t> jobs(size_t(G * nk), 0), loop(size_t(G * nk), 0);
  for (int64_t d = 0; slot_counts && d < P; d++)
    if (group_of[d] >= 0)
      for (int64_t kk = 0; kk < nk; kk++)
        if (st[d * t.K + k_lo + kk] != CYC_JOB_NONE) {
          jobs[size_t(group_of[d] * nk + kk)]++;
          if (il && t.has_row(d)) loop[size_t(group_of[d] * nk + kk)]++;
        }
  for (int64_t gs = 0; gs < G; gs++) {
    const int64_t ns = gt.n_src[size_t(gs)];
    if (!ns) continue;
    for (int64_t gd = 0; gd < G; gd++) {
      const int64_t self = gs == gd ? 1 : 0;
      int64_t* p = pair_counts + (gs * G + gd) * 3;
      p[2] = il * self * ns;
      p[1] = int64_t(cnt[nk * GG + gs * G + gd]) - il * self * int64_t(cnt[(nk + 1) * GG + gs]);
      p[0] = ns * gt.n_dst[size_t(gd)] - p[1] - p[2];
      for (int64_t kk = 0; slot_counts && kk < nk; kk++) {
        int64_t* v = slot_counts + ((gs * G + gd) * nk + kk) * 3;
        v[2] = self * loop[size_t(gs * nk + kk)];
        v[1] = int64_t(cnt[kk * GG + gs * G + gd]);
        v[0] = ns * jobs[size_t(gd * nk + kk)] - v[1] - v[2];
      }
    }
  }
}

// ---- find's page.  c[i]: matching cells of source s_from + i, i < rows (null: none match).  *total = their sum.
// With count_only that is all.  Otherwise sources [s_from, *s_next) are the longest run whose *n records fit into
// cap, offs[i] the first record of source s_from + i; false and `why` when the first source alone does not fit.
inline bool find_page(const cnt_t* c, int64_t rows, int64_t s_from, int64_t cap, bool count_only, int64_t* total, int64_t* n,
                      int64_t* s_next, std::vector<cnt_t>& offs, std::string& why) {
  *total = 0, *n = 0, *s_next = s_from;
  offs.assign(1, 0);
  if (!c) {  // (the page is every source)
    if (!count_only) *s_next = s_from + rows;
    return true;
  }
  for (int64_t i = 0; i < rows; i++) *total += int64_t(c[i]);
  if (count_only) return true;
  int64_t page = 0;
  while (page < rows && offs.back() + c[page] <= cnt_t(cap)) offs.push_back(offs.back() + c[page++]);
  if (!page && rows) {
    why = "source " + std::to_string(s_from) + " alone has " + std::to_string(c[0]) + " matching cells, more than cap " + std::to_string(cap);
    return false;
  }
  *s_next = s_from + page;
  *n = int64_t(offs.back());
  return true;
}

}  // namespace cyc
