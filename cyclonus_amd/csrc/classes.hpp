// classes.hpp — the host side of cyc_table_classes and cyc_table_cells_at (kernels: dev_classes.hpp; the arithmetic
// that is not a launch: class_terms.hpp).  Part of engine.hip's single translation unit, included after reach.hpp.
//
// One side (sources with FROM planes, destinations with TO planes) runs in two phases over the slot range, each a pair
// of launches per slot without a synchronisation in between: the view plane of the slot, then the row kernel over it.
// Phase 1 hashes every row; the host groups the pods by (hash & mask, status key).  Phase 2 verifies every pod that is
// not its group's smallest against that pod; the pods that fail elect new representatives and are verified again
// (class_terms.hpp), with the full mask normally never.
// Device scratch of a side, freed before the call returns:
//   P * pitch * 8   the view plane V of one slot (pitch = W rounded up to 16 words)
//   P * 8           the row hashes h
//   3 * P * 4       the listed pods, their candidate representatives, and bad
//   nk * W * 16     sources only: the status words of the range (k_find_status_words)
#pragma once

#include "class_terms.hpp"

template <bool TO>
static void view_plane_launch(cyc_table* t, int view, const ViewPlaneArgs& a) {
  const dim3 grid((t->W + TT_WORDS - 1) / TT_WORDS, (t->W + TT_WORDS - 1) / TT_WORDS);
  if (view == CYC_VIEW_INGRESS) k_table_view_plane<TO, CYC_VIEW_INGRESS><<<grid, 1024, 0, t->stream>>>(a);
  else if (view == CYC_VIEW_EGRESS) k_table_view_plane<TO, CYC_VIEW_EGRESS><<<grid, 1024, 0, t->stream>>>(a);
  else k_table_view_plane<TO, CYC_VIEW_COMBINED><<<grid, 1024, 0, t->stream>>>(a);
  HIPCHK(hipGetLastError());
}

// The classes of one side into r (P > 0, a slot range that is not empty).  keys: the destinations' status keys, or null.
template <bool TO>
static void classes_side(cyc_table* t, int view, int64_t k_lo, int64_t k_hi, uint64_t hash_mask, const uint8_t* keys, ClassRounds& r) {
  const uint64_t P = t->P, W = t->W, nk = uint64_t(k_hi - k_lo);
  const uint32_t pitch = uint32_t((W + 15) / 16 * 16);
  DevBuf d_v, d_h, d_pod, d_cand, d_bad, d_stw;
  reach_alloc(d_v, P * pitch * 8, "the view plane");
  reach_alloc(d_h, P * 8, "the row hashes");
  reach_alloc(d_pod, P * 4, "the listed pods");
  reach_alloc(d_cand, P * 4, "the representatives");
  reach_alloc(d_bad, P * 4, "the verification results");
  if (!TO) {
    reach_alloc(d_stw, nk * W * 2 * 8, "the status words");
    FindArgs f{};
    f.t = tile_args(t, k_lo, k_hi);
    f.view = CYC_VIEW_COMBINED, f.code_mask = 0, f.stw = d_stw.as<uint64_t>();
    k_find_status_words<false><<<grid1(nk * W, 256), 256, 0, t->stream>>>(f);
    HIPCHK(hipGetLastError());
  }
  ViewPlaneArgs va{};
  va.P = t->P, va.K = t->K, va.W = t->W, va.pitch = pitch;
  va.t = TablePlanes{t->in, t->eg, t->status};
  va.v = d_v.as<uint64_t>();
  auto plane = [&](uint64_t kk) {
    va.k = uint32_t(k_lo + kk);
    va.stw = TO ? nullptr : d_stw.as<uint64_t>() + kk * W * 2;
    view_plane_launch<TO>(t, view, va);
  };
  RowsArgs ra{};
  ra.P = t->P, ra.W = t->W, ra.pitch = pitch, ra.v = d_v.as<uint64_t>();
  ra.h = d_h.as<uint64_t>(), ra.pod = d_pod.as<uint32_t>(), ra.rep = d_cand.as<uint32_t>(), ra.bad = d_bad.as<uint32_t>();
  constexpr uint32_t rows_per_block = CR_THREADS / 64;
  // phase 1: the hashes
  for (uint64_t kk = 0; kk < nk; kk++) {
    plane(kk);
    ra.first = kk == 0;
    k_rows_hash<<<unsigned((P + rows_per_block - 1) / rows_per_block), CR_THREADS, 0, t->stream>>>(ra);
    HIPCHK(hipGetLastError());
  }
  std::vector<uint64_t> h(size_t(P), 0);
  HIPCHK(hipMemcpyAsync(h.data(), d_h.p, P * 8, hipMemcpyDeviceToHost, t->stream));
  HIPCHK(hipStreamSynchronize(t->stream));
  r.start(int64_t(P), h.data(), hash_mask, keys, int64_t(nk));
  // phase 2: the verification, and again for the pods that failed
  std::vector<uint32_t> bad;
  while (!r.done()) {
    const uint64_t n = r.pod.size();
    HIPCHK(hipMemcpyAsync(d_pod.p, r.pod.data(), n * 4, hipMemcpyHostToDevice, t->stream));
    HIPCHK(hipMemcpyAsync(d_cand.p, r.cand.data(), n * 4, hipMemcpyHostToDevice, t->stream));
    HIPCHK(hipMemsetAsync(d_bad.p, 0, n * 4, t->stream));
    ra.n = uint32_t(n);
    for (uint64_t kk = 0; kk < nk; kk++) {
      plane(kk);
      k_rows_verify<<<unsigned((n + rows_per_block - 1) / rows_per_block), CR_THREADS, 0, t->stream>>>(ra);
      HIPCHK(hipGetLastError());
    }
    bad.resize(size_t(n));
    HIPCHK(hipMemcpyAsync(bad.data(), d_bad.p, n * 4, hipMemcpyDeviceToHost, t->stream));
    HIPCHK(hipStreamSynchronize(t->stream));  // (the list is free again)
    r.refine(bad.data());
  }
}

static int table_classes(cyc_table* t, int view, int64_t k_lo, int64_t k_hi, int32_t* src_class, int32_t* dst_class, int64_t* n_src,
                         int64_t* n_dst, uint64_t hash_mask, int64_t* stats) {
  if (const char* m = view_bad(view)) return table_bad(t, m);
  if (const char* m = slots_bad(t, k_lo, k_hi)) return table_bad(t, m);
  if (!src_class && !dst_class && !n_src && !n_dst) return table_bad(t, "no output requested");
  if (const char* m = reach_table_bad(t)) return table_bad(t, m);
  const int64_t P = t->P, nk = k_hi - k_lo;
  const bool want[2] = {src_class || n_src, dst_class || n_dst};
  int32_t* cls[2] = {src_class, dst_class};
  int64_t* cnt[2] = {n_src, n_dst};
  ClassRounds r[2];
  if (P && nk) {
    const int rc = reach_guarded(t, [&]() -> int {
      if (want[0]) classes_side<false>(t, view, k_lo, k_hi, hash_mask, nullptr, r[0]);
      if (want[1]) {
        std::vector<uint8_t> st(size_t(P) * t->K), keys;
        HIPCHK(hipMemcpyAsync(st.data(), t->status, st.size(), hipMemcpyDeviceToHost, t->stream));
        HIPCHK(hipStreamSynchronize(t->stream));
        class_status_keys(view, st.data(), P, t->K, k_lo, nk, keys);
        classes_side<true>(t, view, k_lo, k_hi, hash_mask, keys.data(), r[1]);
      }
      return (int)CYC_OK;
    });
    if (rc != CYC_OK) return rc;
  }
  // (an empty slot range: every pod is class 0; no pods: nothing to write)
  try {
    for (int x = 0; x < 2; x++) {
      if (!want[x]) continue;
      if (P && !nk) r[x].rep.assign(size_t(P), 0);
      const int64_t n = r[x].number(cls[x]);
      if (cnt[x]) *cnt[x] = n;
    }
  } catch (std::bad_alloc&) {
    return t->err = "host allocation failed", (int)CYC_ERR_OOM;
  }
  if (stats)
    for (int x = 0; x < 2; x++) stats[2 * x] = r[x].rounds, stats[2 * x + 1] = r[x].failed;
  return (int)CYC_OK;
}

static int table_cells_at(cyc_table* t, const int32_t* srcs, int64_t n_s, const int32_t* dsts, int64_t n_d, int64_t k_lo, int64_t k_hi,
                          uint8_t* ingress, uint8_t* egress, uint8_t* combined) {
  if (const char* m = slots_bad(t, k_lo, k_hi)) return table_bad(t, m);
  std::string why;
  if (const char* m = pod_list_bad(t->P, "srcs", srcs, n_s, why)) return table_bad(t, m);
  if (const char* m = pod_list_bad(t->P, "dsts", dsts, n_d, why)) return table_bad(t, m);
  if (!ingress && !egress && !combined) return table_bad(t, "no output requested");
  const uint64_t nk = uint64_t(k_hi - k_lo);
  if (!n_s || !n_d || !nk) return (int)CYC_OK;
  // cyc_table_cells' row rules, entry by entry
  const bool src = t->partition == CYC_ROWS_SOURCE;
  const bool need_d = !src && (ingress || combined), need_s = egress || combined || (src && ingress);
  for (int64_t i = 0; need_d && i < n_d; i++)
    if (!t->has_row(dsts[i])) return table_bad(t, "ingress cells need destinations inside the table's rows");
  for (int64_t i = 0; need_s && i < n_s; i++)
    if (!t->has_row(srcs[i]))
      return table_bad(t, src ? "cells of a source-row table need sources inside its rows" : "egress cells need sources inside the table's rows");
  if (n_s > INT32_MAX || n_d > INT32_MAX || uint64_t(n_s) > (uint64_t(1) << 62) / uint64_t(n_d) / nk) return t->err = "more cells than a device allocation holds", (int)CYC_ERR_OOM;
  const uint64_t n = uint64_t(n_s) * uint64_t(n_d) * nk;
  return reach_guarded(t, [&]() -> int {
    DevBuf o[3], d_s, d_d;
    uint8_t* host[3] = {ingress, egress, combined};
    for (int x = 0; x < 3; x++)
      if (host[x]) reach_alloc(o[x], n, "the cells");
    reach_alloc(d_s, uint64_t(n_s) * 4, "the source list");
    reach_alloc(d_d, uint64_t(n_d) * 4, "the destination list");
    HIPCHK(hipMemcpyAsync(d_s.p, srcs, uint64_t(n_s) * 4, hipMemcpyHostToDevice, t->stream));
    HIPCHK(hipMemcpyAsync(d_d.p, dsts, uint64_t(n_d) * 4, hipMemcpyHostToDevice, t->stream));
    CellsAtArgs b{};
    CellArgs& a = b.c;
    a.K = t->K, a.W = t->W, a.w0 = t->w0, a.WA = t->wa;
    a.row_lo = uint32_t(t->row_lo), a.row_hi = uint32_t(t->row_hi), a.src = src ? 1u : 0u;
    a.in = t->in, a.eg = t->eg, a.status = t->status;
    a.k_lo = uint32_t(k_lo), a.nd = uint32_t(n_d), a.nk = uint32_t(nk), a.n = n;
    a.o_in = o[0].as<uint8_t>(), a.o_eg = o[1].as<uint8_t>(), a.o_comb = o[2].as<uint8_t>();
    b.srcs = d_s.as<int32_t>(), b.dsts = d_d.as<int32_t>();
    k_table_cells_at<<<grid1(n, 256), 256, 0, t->stream>>>(b);
    HIPCHK(hipGetLastError());
    for (int x = 0; x < 3; x++)
      if (host[x]) HIPCHK(hipMemcpyAsync(host[x], o[x].p, n, hipMemcpyDeviceToHost, t->stream));
    HIPCHK(hipStreamSynchronize(t->stream));
    return (int)CYC_OK;
  });
}
