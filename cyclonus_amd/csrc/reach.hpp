// reach.hpp — the host side of cyc_table_adjacency and cyc_table_reach (kernels: dev_reach.hpp; the arithmetic that is
// not a launch: reach_terms.hpp).  Part of engine.hip's single translation unit, included after table.hpp.
#pragma once

#include "reach_terms.hpp"

// Both calls take a table that answers every cell with planes [P][K][W]: all target rows, or source rows [0, P)
// (whose ingress window is the whole row).  A shard is refused like a partial target-row table.
static const char* reach_table_bad(const cyc_table* t) {
  if (t->row_lo == 0 && t->row_hi == int64_t(t->P)) return nullptr;
  return "ingress cells need destinations inside the table's rows";
}
static const char* reach_direction_bad(int direction) {
  return direction != CYC_REACH_FROM && direction != CYC_REACH_TO ? "unknown direction" : nullptr;
}

namespace {
struct ReachOom {  // a scratch allocation failed (CYC_ERR_OOM)
  std::string msg;
};
}  // namespace
static void reach_alloc(DevBuf& b, uint64_t bytes, const char* what) {
  b.alloc(0);
  if (!bytes) return;
  void* p = nullptr;
  if (hipMalloc(&p, bytes) != hipSuccess) {
    (void)hipGetLastError();
    throw ReachOom{std::string("device allocation of ") + std::to_string(bytes) + " bytes for " + what + " failed"};
  }
  b.p = p, b.bytes = bytes;
}

// The adjacency plane of slots [k_lo, k_hi) into d_adj ([P][pitch]), enqueued on the table's stream.  `stw` keeps the
// status words of the FROM orientation until the caller has synchronised.
static void adjacency_launch(cyc_table* t, int64_t k_lo, int64_t k_hi, int direction, uint64_t* d_adj, uint32_t pitch, DevBuf& stw) {
  if (!t->P) return;
  AdjArgs a{};
  a.P = t->P, a.K = t->K, a.W = t->W, a.k_lo = uint32_t(k_lo), a.nk = uint32_t(k_hi - k_lo), a.pitch = pitch;
  a.t = TablePlanes{t->in, t->eg, t->status};
  a.adj = d_adj;
  const dim3 grid((t->W + TT_WORDS - 1) / TT_WORDS, (t->W + TT_WORDS - 1) / TT_WORDS);
  if (direction == CYC_REACH_TO) {
    k_table_adjacency<true><<<grid, 1024, 0, t->stream>>>(a);
  } else {
    const uint64_t n_stw = uint64_t(a.nk) * t->W;
    if (n_stw) {
      reach_alloc(stw, n_stw * 2 * 8, "the status words");
      FindArgs f{};
      f.t = tile_args(t, k_lo, k_hi);
      f.view = CYC_VIEW_COMBINED, f.code_mask = 0, f.stw = stw.as<uint64_t>();
      k_find_status_words<false><<<grid1(n_stw, 256), 256, 0, t->stream>>>(f);
      HIPCHK(hipGetLastError());
    }
    a.stw = stw.as<uint64_t>();
    k_table_adjacency<false><<<grid, 1024, 0, t->stream>>>(a);
  }
  HIPCHK(hipGetLastError());
}

template <class F>
static int reach_guarded(cyc_table* t, F&& f) {
  return table_guarded(t, [&]() -> int {
    try {
      return f();
    } catch (ReachOom& o) {
      return t->err = o.msg, (int)CYC_ERR_OOM;
    }
  });
}

static int table_adjacency(cyc_table* t, int64_t k_lo, int64_t k_hi, int direction, uint64_t* d_adj) {
  if (const char* m = reach_direction_bad(direction)) return table_bad(t, m);
  if (const char* m = slots_bad(t, k_lo, k_hi)) return table_bad(t, m);
  if (const char* m = reach_table_bad(t)) return table_bad(t, m);
  if (reinterpret_cast<uintptr_t>(d_adj) % 8) return table_bad(t, "d_adj is not 8-byte aligned");
  if (!t->P) return (int)CYC_OK;  // (a plane of no bytes)
  if (!d_adj) return table_bad(t, "null d_adj");
  return reach_guarded(t, [&]() -> int {
    DevBuf stw;
    adjacency_launch(t, k_lo, k_hi, direction, d_adj, t->W, stw);
    HIPCHK(hipStreamSynchronize(t->stream));
    return (int)CYC_OK;
  });
}

static int table_reach(cyc_table* t, int64_t k_lo, int64_t k_hi, int direction, const int64_t* seed_off, const int32_t* seeds,
                       int64_t n_sets, int64_t max_hops, uint64_t* reach, int32_t* hops, int64_t* levels) {
  if (const char* m = reach_direction_bad(direction)) return table_bad(t, m);
  if (const char* m = slots_bad(t, k_lo, k_hi)) return table_bad(t, m);
  if (const char* m = reach_table_bad(t)) return table_bad(t, m);
  std::string why;
  if (const char* m = reach_seeds_bad(t->P, seed_off, seeds, n_sets, why)) return table_bad(t, m);
  if (!reach && !hops && !levels) return table_bad(t, "no output requested");
  if (const char* m = reach_size_bad(t->W, n_sets)) return table_bad(t, m);
  if (!n_sets) return (int)CYC_OK;
  const uint64_t P = t->P, W = t->W, n_words = uint64_t(n_sets) * W;
  std::vector<uint64_t> bits;
  std::vector<int64_t> lv;
  try {
    reach_seed_bits(int64_t(W), seed_off, seeds, n_sets, bits, lv);
  } catch (std::bad_alloc&) {
    return t->err = "host allocation failed", (int)CYC_ERR_OOM;
  }
  if (!P) {  // (no pods: every set is empty)
    if (levels) std::copy(lv.begin(), lv.end(), levels);
    return (int)CYC_OK;
  }
  return reach_guarded(t, [&]() -> int {
    // scratch of the call: the adjacency plane with its rows padded to whole 128-byte lines (the step's 16-byte
    // loads), visited and the two frontiers, the hop values when they are asked for, two counters per set
    const uint32_t pitch = uint32_t((W + 15) / 16 * 16);
    DevBuf d_adj, d_stw, d_vis, d_front[2], d_hops, d_cnt;
    reach_alloc(d_adj, P * pitch * 8, "the adjacency plane");
    reach_alloc(d_vis, n_words * 8, "the visited sets");
    reach_alloc(d_front[0], n_words * 8, "a frontier");
    reach_alloc(d_front[1], n_words * 8, "a frontier");
    reach_alloc(d_cnt, uint64_t(n_sets) * 8, "the counters");
    if (hops) reach_alloc(d_hops, uint64_t(n_sets) * P * 4, "the hop values");
    adjacency_launch(t, k_lo, k_hi, direction, d_adj.as<uint64_t>(), pitch, d_stw);
    HIPCHK(hipMemcpyAsync(d_vis.p, bits.data(), n_words * 8, hipMemcpyHostToDevice, t->stream));
    HIPCHK(hipMemcpyAsync(d_front[0].p, bits.data(), n_words * 8, hipMemcpyHostToDevice, t->stream));
    ReachArgs a{};
    a.P = uint32_t(P), a.W = uint32_t(W), a.pitch = pitch, a.chunks = uint32_t((W + RS_CHUNK - 1) / RS_CHUNK);
    a.adj = d_adj.as<uint64_t>(), a.visited = d_vis.as<uint64_t>(), a.hops = d_hops.as<int32_t>(), a.cnt = d_cnt.as<cnt_t>();
    if (hops) {
      HIPCHK(hipMemsetAsync(d_hops.p, 0xFF, uint64_t(n_sets) * P * 4, t->stream));  // -1: not reached
      a.front = d_front[0].as<uint64_t>();
      k_reach_seed_hops<<<grid1(n_words, 256), 256, 0, t->stream>>>(a, n_words);
      HIPCHK(hipGetLastError());
    }
    // a launch per hop; it ends at max_hops or when no set found a new pod (one counter read per hop)
    std::vector<cnt_t> cnt(size_t(n_sets), 0);
    int cur = 0;
    for (int64_t hop = 1; max_hops < 0 || hop <= max_hops; hop++, cur ^= 1) {
      HIPCHK(hipMemsetAsync(d_cnt.p, 0, uint64_t(n_sets) * 8, t->stream));
      a.hop = int32_t(hop), a.front = d_front[cur].as<uint64_t>(), a.next = d_front[cur ^ 1].as<uint64_t>();
      k_reach_step<<<unsigned(uint64_t(n_sets) * a.chunks), RS_THREADS, 0, t->stream>>>(a);
      HIPCHK(hipGetLastError());
      HIPCHK(hipMemcpyAsync(cnt.data(), d_cnt.p, uint64_t(n_sets) * 8, hipMemcpyDeviceToHost, t->stream));
      HIPCHK(hipStreamSynchronize(t->stream));
      if (!reach_levels(cnt.data(), n_sets, hop, lv.data())) break;
    }
    if (reach) HIPCHK(hipMemcpyAsync(reach, d_vis.p, n_words * 8, hipMemcpyDeviceToHost, t->stream));
    if (hops) HIPCHK(hipMemcpyAsync(hops, d_hops.p, uint64_t(n_sets) * P * 4, hipMemcpyDeviceToHost, t->stream));
    HIPCHK(hipStreamSynchronize(t->stream));
    if (levels) std::copy(lv.begin(), lv.end(), levels);
    return (int)CYC_OK;
  });
}
