// zone_graph.hpp — the host side of cyc_table_zone_graph (kernels: dev_zone_graph.hpp; the arithmetic that is not a
// launch: zone_terms.hpp).  Part of engine.hip's single translation unit, included after closure.hpp.
// Device scratch of a call beyond cyc_table_zones', freed before it returns:
//   Z * 4             the zones' smallest pods
//   Z * zpitch * 8    the zone reach plane (zpitch = ceil(Z / 64) rounded up to 16 words), for the edges, tiers or d_zreach
//   Z * zpitch * 8    the cover plane, and Z * 8 the rows' edge counts and then offsets, for the edges or tiers
//   n_edges * 8       the edge list, when it is listed
#pragma once

#include "zone_terms.hpp"

static int table_zone_graph(cyc_table* t, int64_t k_lo, int64_t k_hi, int32_t* zone, int64_t* n_zones, int32_t* rep_out, int64_t* size_out,
                            int32_t* tier_out, cyc_zone_edge* edges, int64_t edge_cap, int64_t* n_edges, uint64_t* d_zreach,
                            int64_t zreach_words) {
  if (const char* m = closure_table_bad(t, k_lo, k_hi)) return table_bad(t, m);
  if (const char* m = zone_graph_args_bad(n_zones, edges, edge_cap, n_edges, d_zreach, zreach_words)) return table_bad(t, m);
  const uint64_t P = t->P;
  if (!P) {  // (no pod: nothing to write but the two counts)
    *n_zones = 0;
    if (n_edges) *n_edges = 0;
    return (int)CYC_OK;
  }
  return reach_guarded(t, [&]() -> int {
    ClosureScratch s;
    DevBuf d_rep, d_from, d_to, d_head, d_r, d_cover, d_cnt, d_edges;
    std::vector<uint32_t> rep(size_t(P), 0), head;
    std::vector<int32_t> id, tier;
    std::vector<int64_t> size;
    std::vector<cnt_t> cnt;
    std::vector<cyc_zone_edge> list;
    std::string why;
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
    HIPCHK(hipStreamSynchronize(t->stream));
    if (const char* m = zone_reps_bad(rep.data(), int64_t(P), why)) return t->err = m, (int)CYC_ERR_HIP;
    id.reserve(size_t(P));
    const int64_t Z = zone_number(rep.data(), int64_t(P), nullptr, id);
    zone_heads(rep.data(), int64_t(P), head);
    if (d_zreach)
      if (const char* m = zone_zreach_cap_bad(zreach_words, Z, why)) return *n_zones = Z, t->err = m, (int)CYC_ERR_ARG;
    const bool want_list = edges || tier_out, want_cover = want_list || n_edges;
    uint64_t total = 0;
    ZoneGraphArgs g{};
    g.Z = uint32_t(Z), g.Wz = uint32_t(zone_words(uint64_t(Z))), g.zpitch = uint32_t(zone_pitch(uint64_t(Z))), g.pitch = s.a.pitch;
    g.c = s.a.c;
    if (want_cover || d_zreach) {
      reach_alloc(d_head, uint64_t(Z) * 4, "the zones' smallest pods");
      reach_alloc(d_r, uint64_t(Z) * g.zpitch * 8, "the zone reach plane");
      HIPCHK(hipMemcpyAsync(d_head.p, head.data(), uint64_t(Z) * 4, hipMemcpyHostToDevice, t->stream));
      g.rep = d_head.as<uint32_t>(), g.r = d_r.as<uint64_t>();
      k_zone_compress<<<grid1(uint64_t(Z) * g.zpitch, 4), 256, 0, t->stream>>>(g);
      HIPCHK(hipGetLastError());
    }
    if (want_cover) {
      reach_alloc(d_cover, uint64_t(Z) * g.zpitch * 8, "the cover plane");
      reach_alloc(d_cnt, uint64_t(Z) * 8, "the rows' edge counts");
      cnt.resize(size_t(Z));
      g.cover = d_cover.as<uint64_t>(), g.cnt = d_cnt.as<cnt_t>();
      const dim3 cover_grid((g.zpitch + ZC_CHUNK - 1) / ZC_CHUNK, (g.Z + ZC_ROWS - 1) / ZC_ROWS);
      k_zone_cover<<<cover_grid, ZC_THREADS, 0, t->stream>>>(g);
      HIPCHK(hipGetLastError());
      k_zone_counts<<<grid1(uint64_t(Z), 4), 256, 0, t->stream>>>(g);
      HIPCHK(hipGetLastError());
      HIPCHK(hipMemcpyAsync(cnt.data(), d_cnt.p, uint64_t(Z) * 8, hipMemcpyDeviceToHost, t->stream));
      HIPCHK(hipStreamSynchronize(t->stream));
      total = zone_offsets(cnt.data(), Z);
      if (edges)
        if (const char* m = zone_edge_cap_bad(edge_cap, total, why)) return *n_zones = Z, *n_edges = int64_t(total), t->err = m, (int)CYC_ERR_ARG;
    }
    if (want_list) {
      list.resize(size_t(total));
      if (total) {
        reach_alloc(d_edges, total * 8, "the cover edges");
        HIPCHK(hipMemcpyAsync(d_cnt.p, cnt.data(), uint64_t(Z) * 8, hipMemcpyHostToDevice, t->stream));
        g.total = total, g.edges = d_edges.as<int2>();
        k_zone_edges<<<grid1(uint64_t(Z), 4), 256, 0, t->stream>>>(g);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(list.data(), d_edges.p, total * 8, hipMemcpyDeviceToHost, t->stream));
        HIPCHK(hipStreamSynchronize(t->stream));
      }
      if (const char* m = zone_edges_bad(list.data(), int64_t(total), Z, why)) return t->err = m, (int)CYC_ERR_HIP;
      if (tier_out)
        if (const char* m = zone_tiers(list.data(), int64_t(total), Z, tier, why)) return t->err = m, (int)CYC_ERR_HIP;
    }
    if (size_out) zone_sizes(id.data(), int64_t(P), Z, size);
    if (d_zreach) {  // the caller's rows have no padding
      k_zone_copy<<<grid1(uint64_t(Z) * g.Wz, 256), 256, 0, t->stream>>>(g, d_zreach);
      HIPCHK(hipGetLastError());
      HIPCHK(hipStreamSynchronize(t->stream));
    }
    // (nothing of the caller's host arrays is written before the last thing that can fail)
    *n_zones = Z;
    if (n_edges) *n_edges = int64_t(total);
    if (zone) std::copy(id.begin(), id.end(), zone);
    if (rep_out) std::copy(head.begin(), head.end(), rep_out);
    if (size_out) std::copy(size.begin(), size.end(), size_out);
    if (tier_out) std::copy(tier.begin(), tier.end(), tier_out);
    if (edges) std::copy(list.begin(), list.end(), edges);
    return (int)CYC_OK;
  });
}
