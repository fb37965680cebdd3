// closure.hpp — the host side of cyc_table_closure and cyc_table_zones (kernels: dev_closure.hpp; the arithmetic that is
// not a launch: closure_terms.hpp).  Part of engine.hip's single translation unit, included after reach.hpp.
// Device scratch of a call, freed before it returns:
//   P * pitch * 8    the closure plane (pitch = W rounded up to 16 words)
//   64 * pitch * 8   the pivot panel
//   P * 8            the snapshot of the pivot word
//   P * 8            closure with n_reach: the row counts;  zones: P * 20, the representatives and the two counts
//   nk * W * 16      FROM: the status words of the range (k_find_status_words)
#pragma once

#include "closure_terms.hpp"

namespace {
struct ClosureScratch {
  DevBuf c, panel, mcol, stw;
  ClosureArgs a{};
};
}  // namespace

// The closure of slots [k_lo, k_hi) into s.c ([P][pitch]), enqueued on the table's stream (P > 0): the adjacency plane,
// the start, then two launches per pivot word.  An empty slot range has no edge: the start's identity is the closure.
static void closure_launch(cyc_table* t, int64_t k_lo, int64_t k_hi, int direction, ClosureScratch& s) {
  const uint64_t P = t->P, W = t->W, pitch = closure_pitch(W);
  reach_alloc(s.c, P * pitch * 8, "the closure plane");
  reach_alloc(s.panel, 64 * pitch * 8, "the pivot panel");
  reach_alloc(s.mcol, P * 8, "the pivot word's snapshot");
  ClosureArgs& a = s.a;
  a.P = t->P, a.W = t->W, a.pitch = uint32_t(pitch);
  a.c = s.c.as<uint64_t>(), a.panel = s.panel.as<uint64_t>(), a.mcol = s.mcol.as<uint64_t>();
  adjacency_launch(t, k_lo, k_hi, direction, a.c, a.pitch, s.stw);
  k_closure_start<<<grid1(P, 256), 256, 0, t->stream>>>(a);
  HIPCHK(hipGetLastError());
  if (k_hi == k_lo) return;
  a.panel_blocks = uint32_t((pitch / CP_WORDS + CP_WAVES - 1) / CP_WAVES);
  const unsigned snap_blocks = unsigned((P + CP_WAVES * 64 - 1) / (CP_WAVES * 64));
  const dim3 update_grid(unsigned((pitch + CU_CHUNK - 1) / CU_CHUNK), unsigned((P + CU_ROWS - 1) / CU_ROWS));
  for (uint32_t kb = 0; kb < W; kb++) {
    a.kb = kb;
    k_closure_panel<<<a.panel_blocks + snap_blocks, CP_WAVES * 64, 0, t->stream>>>(a);
    k_closure_update<<<update_grid, CU_THREADS, 0, t->stream>>>(a);
  }
  HIPCHK(hipGetLastError());
}

// what the two calls refuse alike; nullptr when the arguments are fine
static const char* closure_table_bad(const cyc_table* t, int64_t k_lo, int64_t k_hi) {
  if (const char* m = slots_bad(t, k_lo, k_hi)) return m;
  return reach_table_bad(t);
}

static int table_closure(cyc_table* t, int64_t k_lo, int64_t k_hi, int direction, uint64_t* d_closure, int64_t* n_reach) {
  if (const char* m = reach_direction_bad(direction)) return table_bad(t, m);
  if (const char* m = closure_table_bad(t, k_lo, k_hi)) return table_bad(t, m);
  if (const char* m = closure_outputs_bad(d_closure, n_reach)) return table_bad(t, m);
  const uint64_t P = t->P;
  if (!P) return (int)CYC_OK;  // (a plane of no bytes, no pod to count for)
  return reach_guarded(t, [&]() -> int {
    ClosureScratch s;
    DevBuf d_n;
    std::vector<cnt_t> n;
    if (n_reach) reach_alloc(d_n, P * 8, "the row counts"), n.resize(size_t(P));
    closure_launch(t, k_lo, k_hi, direction, s);
    if (n_reach) {
      k_closure_counts<<<grid1(P, 4), 256, 0, t->stream>>>(s.a, d_n.as<cnt_t>());
      HIPCHK(hipGetLastError());
      HIPCHK(hipMemcpyAsync(n.data(), d_n.p, P * 8, hipMemcpyDeviceToHost, t->stream));
    }
    if (d_closure) {  // the caller's rows have no padding
      k_closure_copy<<<grid1(P * t->W, 256), 256, 0, t->stream>>>(s.a, d_closure);
      HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(t->stream));
    if (n_reach) std::copy(n.begin(), n.end(), n_reach);
    return (int)CYC_OK;
  });
}

static int table_zones(cyc_table* t, int64_t k_lo, int64_t k_hi, int32_t* zone, int64_t* n_zones, int64_t* n_from, int64_t* n_to) {
  if (const char* m = closure_table_bad(t, k_lo, k_hi)) return table_bad(t, m);
  if (const char* m = zones_outputs_bad(zone, n_zones, n_from, n_to)) return table_bad(t, m);
  const uint64_t P = t->P;
  if (!P) {  // (no pod: nothing to write but the count)
    if (n_zones) *n_zones = 0;
    return (int)CYC_OK;
  }
  return reach_guarded(t, [&]() -> int {
    ClosureScratch s;
    DevBuf d_rep, d_from, d_to;
    std::vector<uint32_t> rep(size_t(P), 0);
    std::vector<cnt_t> from(size_t(P), 0), to(size_t(P), 0);
    std::vector<int32_t> id;
    reach_alloc(d_rep, P * 4, "the representatives");
    reach_alloc(d_from, P * 8, "the row counts");
    reach_alloc(d_to, P * 8, "the column counts");
    closure_launch(t, k_lo, k_hi, CYC_REACH_FROM, s);
    ZoneArgs z{};
    z.P = t->P, z.W = t->W, z.pitch = s.a.pitch, z.c = s.a.c;
    z.rep = d_rep.as<uint32_t>(), z.n_from = d_from.as<cnt_t>(), z.n_to = d_to.as<cnt_t>();
    k_closure_zones<<<(t->W + TT_WORDS - 1) / TT_WORDS, 1024, 0, t->stream>>>(z);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(rep.data(), d_rep.p, P * 4, hipMemcpyDeviceToHost, t->stream));
    HIPCHK(hipMemcpyAsync(from.data(), d_from.p, P * 8, hipMemcpyDeviceToHost, t->stream));
    HIPCHK(hipMemcpyAsync(to.data(), d_to.p, P * 8, hipMemcpyDeviceToHost, t->stream));
    HIPCHK(hipStreamSynchronize(t->stream));
    std::string why;
    if (const char* m = zone_reps_bad(rep.data(), int64_t(P), why)) return t->err = m, (int)CYC_ERR_HIP;
    id.reserve(size_t(P));  // (nothing of the caller's is written before the last thing that can fail)
    const int64_t n = zone_number(rep.data(), int64_t(P), zone, id);
    if (n_zones) *n_zones = n;
    if (n_from) std::copy(from.begin(), from.end(), n_from);
    if (n_to) std::copy(to.begin(), to.end(), n_to);
    return (int)CYC_OK;
  });
}
