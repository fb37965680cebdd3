// table.hpp — device-resident tables: the host side of the cyc_table_* entry points (kernels: dev_table.hpp,
// dev_query.hpp; the arithmetic on what they deliver: table_terms.hpp).  Part of engine.hip's single translation
// unit, included after enqueue.hpp.  Failures of an entry point that has a table land in cyc_table_error(t).
#pragma once

#include "table_terms.hpp"

static_assert(GROUP_TILE_WORDS == TT_WORDS, "GroupTables numbers the groups of k_table_group_tiles' blocks");

struct cyc_table : TableShape {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  const uint64_t *in = nullptr, *eg = nullptr;
  const uint8_t* status = nullptr;
  DevBuf own_in, own_eg, own_st;  // cyc_table_run: the table owns its planes
};

// Plane shapes of rows [lo, hi) under a partition: ingress rows, words per ingress row slot, egress
// rows, words per egress row slot, first word of the ingress window.
static bool rows_layout(const cyc_ctx* c, int part, int64_t lo, int64_t hi, int64_t v[5], std::string& why) {
  const int64_t P = c->pb.P, W = c->pb.W;
  // a context prepared for batched blocks has per-block slabs, not row planes (cyc_probe_run_blocks)
  if (!c->pb.blocks.empty()) return why = "context prepared for blocks: use cyc_probe_run_blocks", false;
  if (part != CYC_ROWS_TARGET && part != CYC_ROWS_SOURCE) return why = "unknown partition", false;
  if (lo < 0 || hi > P || lo > hi) return why = "row range out of bounds", false;
  if (part == CYC_ROWS_SOURCE && (lo % 64 || (hi % 64 && hi != P)))
    return why = "source rows: row_lo must be a multiple of 64, row_hi too unless it is the pod count", false;
  const bool src = part == CYC_ROWS_SOURCE;
  const int64_t wa = src ? (hi > lo ? (hi + 63) / 64 - lo / 64 : 0) : W;
  v[0] = src ? P : hi - lo, v[1] = wa, v[2] = hi - lo, v[3] = W, v[4] = src ? lo / 64 : 0;
  return true;
}

static int table_new(cyc_ctx* c, int part, int64_t lo, int64_t hi, cyc_table** out) {
  int64_t v[5];
  std::string why;
  if (!rows_layout(c, part, lo, hi, v, why)) return fail(c, CYC_ERR_ARG, why);
  auto* t = new cyc_table();
  t->device = c->device;
  t->P = c->pb.P, t->K = c->pb.K, t->W = c->pb.W;
  t->row_lo = lo, t->row_hi = hi, t->partition = part;
  t->w0 = uint32_t(v[4]), t->wa = uint32_t(v[1]);
  *out = t;
  return (int)CYC_OK;
}

// cyc_table_run_rows: the probe's planes of rows [lo, hi) as a table that owns them
static int table_run(cyc_ctx* c, int part, int64_t lo, int64_t hi, cyc_table** out) {
  return guarded(c, [&]() -> int {
    DeviceGuard dg(c->device);
    cyc_table* t = nullptr;
    int rc = table_new(c, part, lo, hi, &t);
    if (rc != CYC_OK) return rc;
    std::unique_ptr<cyc_table> hold(t);
    const uint64_t words_in = uint64_t(part == CYC_ROWS_SOURCE ? c->pb.P : hi - lo) * c->pb.K * t->wa;
    const uint64_t words_eg = uint64_t(hi - lo) * c->pb.K * c->pb.W;
    t->own_in.alloc(std::max<uint64_t>(words_in * 8, 16));
    t->own_eg.alloc(std::max<uint64_t>(words_eg * 8, 16));
    t->own_st.alloc(std::max<uint64_t>(uint64_t(c->pb.P) * c->pb.K, 16));
    t->in = t->own_in.as<uint64_t>(), t->eg = t->own_eg.as<uint64_t>(), t->status = t->own_st.as<uint8_t>();
    rc = run_pipeline(c, c->stream, t->own_in.as<uint64_t>(), t->own_eg.as<uint64_t>(), t->own_st.as<uint8_t>(), lo, hi,
                      false, part == CYC_ROWS_SOURCE);
    HIPCHK(hipStreamSynchronize(c->stream));
    if (rc != CYC_OK) return rc;
    *out = hold.release();
    return (int)CYC_OK;
  });
}

// ---- shared: the refusal, the argument checks (the message, or nullptr when fine), the guarded scope, the counted pass
static int table_bad(cyc_table* t, const std::string& m) {
  return t->err = m, (int)CYC_ERR_ARG;
}
static const char* slots_bad(const cyc_table* t, int64_t k_lo, int64_t k_hi) {
  return k_lo < 0 || k_hi > int64_t(t->K) || k_lo > k_hi ? "slot range out of bounds" : nullptr;
}
// (a partial target-row table holds the ingress rows of its destinations, the egress rows of its sources: no cell has both)
static const char* partial_bad(const cyc_table* t) {
  return t->whole() ? nullptr : "ingress cells need destinations inside the table's rows";
}
static const char* pair_bad(const cyc_table* ta, const cyc_table* tb) {
  if (!tb) return "null table";
  if (ta->device != tb->device || ta->P != tb->P || ta->K != tb->K || ta->partition != tb->partition ||
      ta->row_lo != tb->row_lo || ta->row_hi != tb->row_hi)
    return "cannot compare tables of different devices, shapes, partitions or rows";
  return nullptr;
}
static const char* view_bad(int view) {
  return view != CYC_VIEW_INGRESS && view != CYC_VIEW_EGRESS && view != CYC_VIEW_COMBINED ? "unknown view" : nullptr;
}

// The body of an entry point that uses the device: on the table's device and with its stream (made on first use)
template <class F>
static int table_guarded(cyc_table* t, F&& f) {
  try {
    DeviceGuard dg(t->device);
    if (!t->stream) HIPCHK(hipStreamCreateWithFlags(&t->stream, hipStreamNonBlocking));
    return f();
  } catch (HipErr& h) {
    return t->err = h.msg, (int)CYC_ERR_HIP;
  } catch (std::bad_alloc&) {
    return t->err = "host allocation failed", (int)CYC_ERR_OOM;
  }
}

// One counted pass over the table: n_cnt + n_src zeroed 64-bit device counters (TileArgs::cnt, and behind it src_cnt
// of the per-pod calls), on which `launch` starts its kernels (not at all when the table has no rows: the counters are
// zero); then the two counter arrays and table a's status plane on the host, after one synchronisation.
struct Counted {
  std::vector<cnt_t> cnt, src;
  std::vector<uint8_t> st;
};
template <class F>
static Counted counted_pass(cyc_table* t, uint64_t n_cnt, uint64_t n_src, F&& launch) {
  Counted r;
  r.cnt.assign(n_cnt, 0), r.src.assign(n_src, 0), r.st.assign(size_t(t->P) * t->K, 0);
  DevBuf d_cnt;
  if (n_cnt && t->rows()) {
    d_cnt.alloc((n_cnt + n_src) * 8);
    HIPCHK(hipMemsetAsync(d_cnt.p, 0, (n_cnt + n_src) * 8, t->stream));
    launch(d_cnt.as<cnt_t>(), d_cnt.as<cnt_t>() + n_cnt);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(r.cnt.data(), d_cnt.p, n_cnt * 8, hipMemcpyDeviceToHost, t->stream));
    if (n_src) HIPCHK(hipMemcpyAsync(r.src.data(), d_cnt.as<cnt_t>() + n_cnt, n_src * 8, hipMemcpyDeviceToHost, t->stream));
  }
  if (!r.st.empty()) HIPCHK(hipMemcpyAsync(r.st.data(), t->status, r.st.size(), hipMemcpyDeviceToHost, t->stream));
  HIPCHK(hipStreamSynchronize(t->stream));  // (d_cnt is freed after it)
  return r;
}

// The tile kernel's view of a whole target-row table (sources [0, P)) or of a source-row table; tb: the compare's table b
static TileArgs tile_args(const cyc_table* t, int64_t k_lo, int64_t k_hi, const cyc_table* tb = nullptr, int ignore_loopback = 0) {
  TileArgs a{};
  a.P = t->P, a.K = t->K, a.W = t->W, a.WA = t->wa, a.w0 = t->w0;
  a.s_lo = uint32_t(t->row_lo), a.s_hi = uint32_t(t->row_hi);
  a.k_lo = uint32_t(k_lo), a.nk = uint32_t(k_hi - k_lo);
  a.a = TablePlanes{t->in, t->eg, t->status};
  if (tb) a.b = TablePlanes{tb->in, tb->eg, tb->status};
  a.ignore_loopback = ignore_loopback ? 1u : 0u;
  return a;
}

static dim3 tile_grid(const cyc_table* t, uint32_t source_words = TT_WORDS) {
  return dim3((t->W + TT_WORDS - 1) / TT_WORDS, (t->wa + source_words - 1) / source_words);
}

// ---------------------------------------------------------------- the entry points (t, ta: not null)
static int table_cells(cyc_table* t, int64_t s_lo, int64_t s_hi, int64_t d_lo, int64_t d_hi, int64_t k_lo, int64_t k_hi,
                       uint8_t* ingress, uint8_t* egress, uint8_t* combined) {
  if (s_lo < 0 || s_hi > int64_t(t->P) || s_lo > s_hi || d_lo < 0 || d_hi > int64_t(t->P) || d_lo > d_hi || slots_bad(t, k_lo, k_hi))
    return table_bad(t, "cell range out of bounds");
  // ingress rows are keyed by destination, egress rows by source (include/cyclonus_hip.h); a
  // source-row table holds both directions of its sources' cells
  const bool src = t->partition == CYC_ROWS_SOURCE;
  const bool need_d = !src && (ingress || combined), need_s = egress || combined || (src && ingress);
  if (s_hi > s_lo && d_hi > d_lo && k_hi > k_lo) {
    if (need_d && (d_lo < t->row_lo || d_hi > t->row_hi)) return table_bad(t, "ingress cells need destinations inside the table's rows");
    if (need_s && (s_lo < t->row_lo || s_hi > t->row_hi))
      return table_bad(t, src ? "cells of a source-row table need sources inside its rows" : "egress cells need sources inside the table's rows");
  }
  const uint64_t n = uint64_t(s_hi - s_lo) * uint64_t(d_hi - d_lo) * uint64_t(k_hi - k_lo);
  if (!n) return (int)CYC_OK;
  return table_guarded(t, [&]() -> int {
    DevBuf o[3];
    uint8_t* host[3] = {ingress, egress, combined};
    for (int x = 0; x < 3; x++)
      if (host[x]) o[x].alloc(n);
    CellArgs a{};
    a.K = t->K, a.W = t->W, a.w0 = t->w0, a.WA = t->wa;
    a.row_lo = uint32_t(t->row_lo), a.row_hi = uint32_t(t->row_hi), a.src = src ? 1u : 0u;
    a.in = t->in, a.eg = t->eg, a.status = t->status;
    a.s_lo = uint32_t(s_lo), a.d_lo = uint32_t(d_lo), a.k_lo = uint32_t(k_lo);
    a.nd = uint32_t(d_hi - d_lo), a.nk = uint32_t(k_hi - k_lo), a.n = n;
    a.o_in = o[0].as<uint8_t>(), a.o_eg = o[1].as<uint8_t>(), a.o_comb = o[2].as<uint8_t>();
    k_table_cells<<<grid1(n, 256), 256, 0, t->stream>>>(a);
    HIPCHK(hipGetLastError());
    for (int x = 0; x < 3; x++)
      if (host[x]) HIPCHK(hipMemcpyAsync(host[x], o[x].p, n, hipMemcpyDeviceToHost, t->stream));
    HIPCHK(hipStreamSynchronize(t->stream));
    return (int)CYC_OK;
  });
}

static int table_counts(cyc_table* t, int64_t k_lo, int64_t k_hi, int64_t* ingress, int64_t* egress, int64_t* combined,
                        int64_t* no_job) {
  if (const char* m = slots_bad(t, k_lo, k_hi)) return table_bad(t, m);
  if (!ingress && !egress && !combined && !no_job) return table_bad(t, "no output requested");
  if (const char* m = combined || no_job ? partial_bad(t) : nullptr) return table_bad(t, m);
  const bool whole = t->whole();
  const int64_t nk = k_hi - k_lo, rows = t->rows();
  int64_t* const out[3] = {ingress, egress, combined};
  for (int x = 0; x < 3; x++)
    if (out[x]) std::fill(out[x], out[x] + nk * 6, int64_t(0));
  if (no_job) *no_job = 0;
  if (!nk || !t->P) return (int)CYC_OK;
  return table_guarded(t, [&]() -> int {
    DevBuf d_valid;
    const Counted r = counted_pass(t, uint64_t(whole ? 3 * int64_t(t->P) : 2 * rows) * nk, 0, [&](cnt_t* d_cnt, cnt_t*) {
      if (whole) {
        TileArgs a = tile_args(t, k_lo, k_hi);
        a.cnt = d_cnt;
        k_table_tiles<false><<<tile_grid(t), 1024, 0, t->stream>>>(a);
        return;
      }
      RowCountArgs a{};
      a.P = t->P, a.K = t->K, a.W = t->W, a.row_lo = uint32_t(t->row_lo), a.rows = uint32_t(rows);
      a.k_lo = uint32_t(k_lo), a.nk = uint32_t(nk);
      a.t = TablePlanes{t->in, t->eg, t->status};
      d_valid.alloc(uint64_t(nk) * t->W * 8);
      a.valid = d_valid.as<uint64_t>(), a.cnt = d_cnt;
      k_table_valid_words<<<grid1(uint64_t(nk) * t->W, 256), 256, 0, t->stream>>>(a);
      HIPCHK(hipGetLastError());
      k_table_row_counts<<<unsigned((uint64_t(rows) * nk + 3) / 4), 256, 0, t->stream>>>(a);
    });
    if (whole) counts_whole(*t, r.st.data(), r.cnt.data(), k_lo, nk, out, no_job);
    else counts_partial(*t, r.st.data(), r.cnt.data(), k_lo, nk, ingress, egress);
    return (int)CYC_OK;
  });
}

static int table_pod_counts(cyc_table* t, int view, int64_t k_lo, int64_t k_hi, int64_t* by_src, int64_t* by_dst) {
  if (const char* m = view_bad(view)) return table_bad(t, m);
  if (const char* m = slots_bad(t, k_lo, k_hi)) return table_bad(t, m);
  if (!by_src && !by_dst) return table_bad(t, "no output requested");
  if (const char* m = partial_bad(t)) return table_bad(t, m);
  const int64_t nk = k_hi - k_lo;
  if (!nk || !t->P) return (int)CYC_OK;
  return table_guarded(t, [&]() -> int {
    const Counted r = counted_pass(t, uint64_t(nk) * 3 * t->P, by_src ? uint64_t(nk) * t->wa * 64 : 0, [&](cnt_t* d_cnt, cnt_t* d_src) {
      TileArgs a = tile_args(t, k_lo, k_hi);
      a.cnt = d_cnt, a.src_cnt = d_src, a.view = uint32_t(view);
      if (by_src) k_table_tiles<false, true><<<tile_grid(t), 1024, 0, t->stream>>>(a);
      else k_table_tiles<false><<<tile_grid(t), 1024, 0, t->stream>>>(a);
    });
    pod_counts(*t, r.st.data(), r.cnt.data(), r.src.data(), view, k_lo, nk, by_src, by_dst);
    return (int)CYC_OK;
  });
}

// The compare pass over the tiles: the kernel's per-destination buffer (TileArgs::cnt) and, with `src`, its per-source
// buffer (TileArgs::src_cnt).
static Counted compare_tiles(cyc_table* t, cyc_table* tb, int64_t k_lo, int64_t k_hi, int ignore_loopback, uint64_t* d_diff, bool src) {
  const uint64_t nk = uint64_t(k_hi - k_lo);
  return counted_pass(t, uint64_t(t->P) * (nk + 2), src ? (nk + 1) * t->wa * 64 : 0, [&](cnt_t* d_cnt, cnt_t* d_src) {
    TileArgs a = tile_args(t, k_lo, k_hi, tb, ignore_loopback);
    a.cnt = d_cnt, a.src_cnt = d_src, a.diff = d_diff;
    if (src) k_table_tiles<true, true><<<tile_grid(t, tile_source_words(true, true)), 1024, 0, t->stream>>>(a);
    else k_table_tiles<true><<<tile_grid(t), 1024, 0, t->stream>>>(a);
  });
}

static int table_compare(cyc_table* t, cyc_table* tb, int64_t k_lo, int64_t k_hi, int ignore_loopback, int64_t pair_counts[3],
                         int64_t* slot_counts, int64_t* dst_counts, uint64_t* d_diff) {
  if (const char* m = pair_bad(t, tb)) return table_bad(t, m);
  if (!pair_counts) return table_bad(t, "null pair_counts");
  if (const char* m = slots_bad(t, k_lo, k_hi)) return table_bad(t, m);
  if (const char* m = partial_bad(t)) return table_bad(t, m);
  if (reinterpret_cast<uintptr_t>(d_diff) % 8) return table_bad(t, "d_diff is not 8-byte aligned");
  return table_guarded(t, [&]() -> int {
    const Counted r = compare_tiles(t, tb, k_lo, k_hi, ignore_loopback, d_diff, false);
    compare_pairs(*t, r.cnt.data(), k_hi - k_lo, ignore_loopback ? 1 : 0, pair_counts);
    compare_jobs_by_dst(*t, r.st.data(), r.cnt.data(), k_lo, k_hi - k_lo, ignore_loopback ? 1 : 0, slot_counts, dst_counts);
    return (int)CYC_OK;
  });
}

static int table_pod_compare(cyc_table* t, cyc_table* tb, int64_t k_lo, int64_t k_hi, int ignore_loopback, int64_t* src_pairs,
                             int64_t* dst_pairs, int64_t* src_slots, int64_t* dst_slots) {
  if (const char* m = pair_bad(t, tb)) return table_bad(t, m);
  if (const char* m = slots_bad(t, k_lo, k_hi)) return table_bad(t, m);
  if (const char* m = partial_bad(t)) return table_bad(t, m);
  if (!src_pairs && !dst_pairs && !src_slots && !dst_slots) return table_bad(t, "no output requested");
  return table_guarded(t, [&]() -> int {
    const Counted r = compare_tiles(t, tb, k_lo, k_hi, ignore_loopback, nullptr, src_pairs || src_slots);
    pod_compare(*t, r.st.data(), r.cnt.data(), r.src.data(), k_lo, k_hi - k_lo, ignore_loopback ? 1 : 0, src_pairs, dst_pairs, src_slots,
                dst_slots);
    return (int)CYC_OK;
  });
}

// ---- counts and comparison per pod-group pair
// GroupTables on the device.  Asynchronous: the vectors and `dev` live until the caller has synchronised the stream.
template <class T>
static const T* group_put(DevBuf& b, const T* v, size_t n, hipStream_t st) {
  b.alloc(std::max<size_t>(n * sizeof(T), 16));
  if (n) HIPCHK(hipMemcpyAsync(b.p, v, n * sizeof(T), hipMemcpyHostToDevice, st));
  return b.as<T>();
}
static GroupArgs group_args(const GroupTables& gt, DevBuf dev[10], const TileArgs& tile, const int32_t* group_of, hipStream_t st) {
  GroupArgs g{};
  g.t = tile, g.G = uint32_t(gt.n_src.size());
  g.ent_ptr = group_put(dev[0], gt.ent_ptr.data(), gt.ent_ptr.size(), st);
  g.ent_mask = group_put(dev[1], gt.ent_mask.data(), gt.ent_mask.size(), st);
  g.ent_grp = group_put(dev[2], gt.ent_grp.data(), gt.ent_grp.size(), st);
  g.ent_loc = group_put(dev[3], gt.ent_loc.data(), gt.ent_loc.size(), st);
  g.row_ptr = group_put(dev[4], gt.row_ptr.data(), gt.row_ptr.size(), st);
  g.row_grp = group_put(dev[5], gt.row_grp.data(), gt.row_grp.size(), st);
  g.dst_grp = group_put(dev[6], group_of, tile.P, st);
  g.dst_loc = group_put(dev[7], gt.dst_loc.data(), gt.dst_loc.size(), st);
  g.col_ptr = group_put(dev[8], gt.col_ptr.data(), gt.col_ptr.size(), st);
  g.col_grp = group_put(dev[9], gt.col_grp.data(), gt.col_grp.size(), st);
  return g;
}

static int table_group_counts(cyc_table* t, const int32_t* group_of, int64_t G, int64_t k_lo, int64_t k_hi, int64_t* ingress,
                              int64_t* egress, int64_t* combined, int64_t* no_job) {
  std::string why;
  if (const char* m = group_args_bad(*t, group_of, G, k_lo, k_hi, why)) return table_bad(t, m);
  if (!ingress && !egress && !combined && !no_job) return table_bad(t, "no output requested");
  if (const char* m = partial_bad(t)) return table_bad(t, m);
  const int64_t nk = k_hi - k_lo, GG = G * G;
  int64_t* const out[3] = {ingress, egress, combined};
  for (int x = 0; x < 3; x++)
    if (out[x]) std::fill(out[x], out[x] + GG * nk * 6, int64_t(0));
  if (no_job) std::fill(no_job, no_job + GG, int64_t(0));
  if (!nk || !t->P) return (int)CYC_OK;
  return table_guarded(t, [&]() -> int {
    const GroupTables gt(*t, group_of, G);
    DevBuf dev[10];
    const Counted r = counted_pass(t, uint64_t(nk) * 3 * GG, 0, [&](cnt_t* d_cnt, cnt_t*) {
      GroupArgs a = group_args(gt, dev, tile_args(t, k_lo, k_hi), group_of, t->stream);
      a.t.cnt = d_cnt;
      k_table_group_tiles<false><<<tile_grid(t), 1024, 0, t->stream>>>(a);
    });
    group_counts(*t, r.st.data(), r.cnt.data(), group_of, gt, k_lo, nk, out, no_job);
    return (int)CYC_OK;
  });
}

static int table_group_compare(cyc_table* t, cyc_table* tb, const int32_t* group_of, int64_t G, int64_t k_lo, int64_t k_hi,
                               int ignore_loopback, int64_t* pair_counts, int64_t* slot_counts) {
  if (const char* m = pair_bad(t, tb)) return table_bad(t, m);
  if (!pair_counts) return table_bad(t, "no output requested");
  std::string why;
  if (const char* m = group_args_bad(*t, group_of, G, k_lo, k_hi, why)) return table_bad(t, m);
  if (const char* m = partial_bad(t)) return table_bad(t, m);
  const int64_t nk = k_hi - k_lo, GG = G * G;
  std::fill(pair_counts, pair_counts + GG * 3, int64_t(0));
  if (slot_counts) std::fill(slot_counts, slot_counts + GG * nk * 3, int64_t(0));
  if (!t->P) return (int)CYC_OK;
  return table_guarded(t, [&]() -> int {
    const GroupTables gt(*t, group_of, G);
    DevBuf dev[10];
    const Counted r = counted_pass(t, uint64_t(nk + 1) * GG + G, 0, [&](cnt_t* d_cnt, cnt_t*) {
      GroupArgs a = group_args(gt, dev, tile_args(t, k_lo, k_hi, tb, ignore_loopback), group_of, t->stream);
      a.t.cnt = d_cnt;
      k_table_group_tiles<true><<<tile_grid(t), 1024, 0, t->stream>>>(a);
    });
    group_compare(*t, r.st.data(), r.cnt.data(), group_of, gt, k_lo, nk, ignore_loopback ? 1 : 0, pair_counts, slot_counts);
    return (int)CYC_OK;
  });
}

// ---------------------------------------------------------------- which cells: find and compare_find
static_assert(sizeof(cyc_cell) == 16, "cyc_cell is one 16-byte store");
constexpr uint32_t FIND_LDS_SLOTS = 32;      // 2 KB of words per slot and wave: up to here they fit 64 KB of LDS
constexpr uint32_t FIND_SCRATCH_GRID = 1024;  // beyond, the words live in global scratch and the grid is capped
constexpr uint32_t FIND_EMIT_GRID = 1u << 20;  // waves of the emit kernel; further (source word, block) items by stride

// The shared body of the two entry points: tb == nullptr is find (view, code_mask), otherwise compare_find
// (ignore_loopback).  The callers have checked what only one of them takes.
static int table_find(cyc_table* t, cyc_table* tb, int view, uint32_t code_mask, int ignore_loopback, int64_t k_lo, int64_t k_hi,
                      int64_t s_from, cyc_cell* cells, int64_t cap, int64_t* n, int64_t* s_next, int64_t* total) {
  if (!n || !s_next || !total) return table_bad(t, "null n, s_next or total");
  *n = 0, *total = 0, *s_next = s_from;
  if (const char* m = slots_bad(t, k_lo, k_hi)) return table_bad(t, m);
  if (const char* m = partial_bad(t)) return table_bad(t, m);
  if (s_from < t->row_lo || s_from > t->row_hi) return table_bad(t, "s_from outside the table's rows");
  if (cap < 0) return table_bad(t, "negative cap");
  if (!cells && cap > 0) return table_bad(t, "null cells");
  const int64_t nk = k_hi - k_lo, rows = t->row_hi - s_from;
  std::vector<cnt_t> offs;  // offs[i]: first record of source s_from + i
  std::string why;
  if (!nk || !rows) return find_page(nullptr, rows, s_from, cap, !cells, total, n, s_next, offs, why), (int)CYC_OK;
  return table_guarded(t, [&]() -> int {
    const bool cmp = tb != nullptr;
    FindArgs a{};
    a.t = tile_args(t, k_lo, k_hi, tb, ignore_loopback);
    a.view = uint32_t(view), a.code_mask = code_mask;
    a.NB = (t->W + TT_WORDS - 1) / TT_WORDS;
    a.bx0 = uint32_t((s_from / 64 - t->w0) / TT_WORDS);
    // ---- pass 1: matches per (destination block, source), then per source
    const uint64_t n_src = uint64_t(t->rows()), n_stw = uint64_t(nk) * t->W * 2, n_blk = uint64_t(a.NB) * n_src;
    DevBuf d_cnt, d_stw, d_blk;
    d_cnt.alloc(n_src * 8), d_stw.alloc(n_stw * 8), d_blk.alloc(n_blk * 8);
    HIPCHK(hipMemsetAsync(d_cnt.p, 0, n_src * 8, t->stream));  // (the sources before pass 1's first block)
    a.n_src = uint32_t(n_src), a.t.cnt = d_cnt.as<cnt_t>();
    a.stw = d_stw.as<uint64_t>(), a.blk = d_blk.as<cnt_t>();
    const dim3 grid((t->wa + TT_WORDS - 1) / TT_WORDS - a.bx0, a.NB);
    if (cmp) {
      k_find_status_words<true><<<grid1(n_stw / 2, 256), 256, 0, t->stream>>>(a);
      HIPCHK(hipGetLastError());
      k_table_find_count<true><<<grid, 1024, 0, t->stream>>>(a);
    } else {
      k_find_status_words<false><<<grid1(n_stw / 2, 256), 256, 0, t->stream>>>(a);
      HIPCHK(hipGetLastError());
      k_table_find_count<false><<<grid, 1024, 0, t->stream>>>(a);
    }
    HIPCHK(hipGetLastError());
    k_table_find_scan<<<grid1(n_src - uint64_t(a.bx0) * TT_WORDS * 64, 256), 256, 0, t->stream>>>(a);
    HIPCHK(hipGetLastError());
    std::vector<cnt_t> cnt(n_src);
    HIPCHK(hipMemcpyAsync(cnt.data(), d_cnt.p, n_src * 8, hipMemcpyDeviceToHost, t->stream));
    HIPCHK(hipStreamSynchronize(t->stream));
    // ---- the page: sources [s_from, s_next) are the longest run whose records fit into cap
    if (!find_page(cnt.data() + (s_from - t->row_lo), rows, s_from, cap, !cells, total, n, s_next, offs, why)) return table_bad(t, why);
    if (!*n) return (int)CYC_OK;
    // ---- pass 2: the records of the page
    DevBuf d_offs, d_out, d_scratch;
    d_offs.alloc(offs.size() * 8), d_out.alloc(uint64_t(*n) * sizeof(cyc_cell));
    HIPCHK(hipMemcpyAsync(d_offs.p, offs.data(), offs.size() * 8, hipMemcpyHostToDevice, t->stream));
    a.s_from = uint32_t(s_from), a.s_next = uint32_t(*s_next);
    a.offs = d_offs.as<cnt_t>(), a.out = d_out.as<uint4>();
    // a wave per (source word of the page, destination block); those without a match leave at once
    const uint64_t items = uint64_t((*s_next + 63) / 64 - s_from / 64) * a.NB;
    uint32_t waves = uint32_t(std::min<uint64_t>(items, FIND_EMIT_GRID));
    size_t lds = size_t(nk) * 4 * 64 * 8;
    if (nk > FIND_LDS_SLOTS) {
      waves = std::min(waves, FIND_SCRATCH_GRID);
      d_scratch.alloc(uint64_t(waves) * lds);
      a.scratch = d_scratch.as<uint64_t>();
      lds = 0;
    }
    if (cmp) k_table_find_emit<true><<<waves, 64, lds, t->stream>>>(a);
    else k_table_find_emit<false><<<waves, 64, lds, t->stream>>>(a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(cells, d_out.p, uint64_t(*n) * sizeof(cyc_cell), hipMemcpyDeviceToHost, t->stream));
    HIPCHK(hipStreamSynchronize(t->stream));
    return (int)CYC_OK;
  });
}
