// enqueue.hpp — enqueueing a run: the pipeline pieces, the fused front, the emit, graph capture and replay.
// Part of engine.hip's single translation unit (device bodies inline across stages, host helpers are
// static): included once, by engine.hip, in stage order.
#pragma once

#ifndef CYC_PHASE_GRID
#define CYC_PHASE_GRID 1  // row phases: each class-row launch's grid sized by its phase's identities (0: all)
#endif
#ifndef CYC_PB_REC
#define CYC_PB_REC 1  // identity-set waves read their rows' matcher records (pb_rec); 0: the peers' chains
#endif

// Stage builders.  Each front stage's argument struct is defined next to its *_blk body; x_args fills
// it, block count nb included — the one place the stage's grid is computed.  The two-branch DAG
// launches each struct as a kernel of its own (enq_common, enq_peer_rows), build_front places the
// same structs into the fused launches.
constexpr uint32_t NB_OVER = 0xFFFFFFFFu;  // a range of >= 2^30 blocks: no launch takes it (FrontLaunches::fits)
static uint32_t nb32(uint64_t n) { return n < (1ull << 30) ? uint32_t(n) : NB_OVER; }
template <class A>
static void launch(void (*k)(A), const A& a, hipStream_t st) {
  if (a.nb) k<<<a.nb, 256, 0, st>>>(a);
}
template <class A>
static void launch(void (*k)(PeerCommon, A), const PeerCommon& pc, const A& a, hipStream_t st) {
  if (a.nb) k<<<a.nb, 256, 0, st>>>(pc, a);
}

// the word spans and chunk masks of the IP rows and (pod_spans) of PM builds' sparse pod rows (cnz needs
// no reset; k_ip_rows with panics keeps no spans)
static FillArgs fill_args(cyc_ctx* c, bool pod_spans) {
  FillArgs a{};
  a.p = c->prep.ip_rng.as<uint32_t>();
  a.v = 0xFFFFFFFFu;
  a.n = !c->pb.may_err && (c->range.Ri || c->range.Rr || pod_spans) ? c->pb.peers.size() * 4 : 0;
  a.nb = nb32((a.n + 255) / 256);
  return a;
}
// 1. selectors x label sets (lazy: evaluated where used, no table)
static SelArgs sel_args(cyc_ctx* c, bool lazy) {
  Prepared& prep = c->prep;
  const bool dense = prep.dense_sel;
  SelArgs a{};
  a.S = c->range.n_sel;
  a.L = c->pb.L;
  a.sel_off = prep.sel_off.as<uint32_t>();
  a.reqs = dense ? prep.dreqs.as<DReq>() : prep.reqs.as<DReq>();
  a.req_vals = prep.req_vals.as<uint32_t>();
  a.LVT = prep.lvt.as<uint32_t>();
  a.ls_off = prep.ls_off.as<uint32_t>();
  a.ls_key = prep.ls_key.as<uint32_t>();
  a.ls_val = prep.ls_val.as<uint32_t>();
  a.selres = prep.selres.as<uint8_t>();
  a.sel_list = c->range.sel_list.as<uint32_t>();
  const uint64_t n = uint64_t(a.S) * a.L;
  if (n && !lazy) a.nb = dense ? nb32(uint64_t(a.S) * ((a.L + 256 * SEL_LPT - 1) / (256 * SEL_LPT))) : grid1(n, 256);
  return a;
}
// 3. port matchers x job descriptors, and their descriptor bit rows (direct: from the matchers)
static PortArgs port_args(cyc_ctx* c) {
  Prepared& prep = c->prep;
  PortArgs a{};
  a.M = uint32_t(c->pb.pms.size());
  a.D = uint32_t(std::max<size_t>(c->pb.descs.size(), 1));
  a.pms = prep.pms.as<DPortM>();
  a.pents = prep.pents.as<DPortEntry>();
  a.descs = prep.descs.as<DDesc>();
  a.portok = prep.portok.as<uint8_t>();
  a.nb = a.M && c->pb.descs.size() ? nb32((uint64_t(a.M) * a.D + 255) / 256) : 0u;
  return a;
}
static PortBitsArgs port_bits_args(cyc_ctx* c, const Route& route, bool direct) {
  PortBitsArgs a{};
  a.t = port_args(c);
  a.direct = direct;
  a.portbits = c->prep.portbits.as<uint32_t>();
  a.nb = a.t.nb && route.port_bits ? nb32((uint64_t(a.t.M) + 255) / 256) : 0u;
  return a;
}
// 4. per-slot destination words
static SlotWordsArgs slot_words_args(cyc_ctx* c) {
  Prepared& prep = c->prep;
  SlotWordsArgs a{};
  a.P = c->pb.P;
  a.K = c->pb.K;
  a.W = c->pb.W;
  a.D = uint32_t(std::max<size_t>(c->pb.descs.size(), 1));
  a.slot_desc = prep.slot_desc.as<int32_t>();
  a.slot_status = prep.slot_status.as<uint8_t>();
  a.VALID = prep.VALID.as<uint64_t>();
  a.DESCW = prep.DESCW.as<int32_t>();
  a.DM = prep.DM.as<uint64_t>();
  a.nb = nb32((uint64_t(a.K) * a.W + 3) / 4);
  return a;
}

// 2. peer rows: pod peers in identity space, expanded over word runs (skipped in IDO mode: the class
// rows expand them); IP peers per pod.
static PeerCommon peer_common(cyc_ctx* c) {
  Prepared& prep = c->prep;
  PeerCommon a{};
  a.P = c->pb.P;
  a.W = c->pb.W;
  a.E = prep.dir[1].n;
  a.EW = (a.E + 63) / 64;
  a.PM = prep.PM.as<uint64_t>();
  a.ER = prep.ER.as<uint64_t>();
  a.rng = prep.ip_rng.as<uint32_t>();
  a.cnz = ip_cnz(c);
  a.peers = prep.peers.as<DPeer>();
  a.sv = sel_view(c);
  a.id_ns = prep.dir[1].id_ns.as<uint32_t>();
  a.id_nsls = prep.id_nsls.as<uint32_t>();
  a.id_ls = prep.dir[1].id_ls.as<uint32_t>();
  a.pod_eid = prep.dir[1].pod_id.as<uint32_t>();
  a.pod_ns = prep.pod_ns.as<uint32_t>();
  a.pod_nsls = prep.pod_nsls.as<uint32_t>();
  a.pod_ls = prep.pod_ls.as<uint32_t>();
  a.nsw = prep.ns_words.as<DWordNS>();
  a.words = prep.ip_words.as<DWordIP>();
  a.pod_ip = prep.pod_ip.as<DIP>();
  a.ip_ex = c->range.ip_ex.as<DCidr>();
  a.req_post = prep.req_post.as<uint4>();
  a.post_pods = prep.post_pods.as<uint32_t>();
  return a;
}
// Segment x = 0, 1 of the IP rows and per-pod pod rows: direction x's sub-list [dlo, dhi) with its own
// word window (source shards; a source shard's ingress peers: its sources' words), or — one_window,
// target-row runs — both directions' adjacent sub-lists in segment 0 and nothing in segment 1.
struct PeerSeg {
  int x, dlo, dhi;
  uint32_t w0, nw, c0, nch;  // words [w0, w0 + nw) = 64-word chunks [c0, c0 + nch)
};
static PeerSeg peer_seg(const cyc_ctx* c, bool one_window, int x) {
  PeerSeg s{};
  s.x = x;
  s.dlo = one_window ? 0 : x;
  s.dhi = one_window ? (x ? 0 : 2) : x + 1;
  peer_window(c->range, c->pb.W, one_window ? 1 : x, s.w0, s.nw);
  peer_chunks(c->range, c->pb.W, one_window ? 1 : x, s.c0, s.nch);
  return s;
}
// items: the range plan's work items of the segment (the fused front), when it has them
static IpArgs ip_args(cyc_ctx* c, const PeerSeg& s, bool items) {
  RangePlan& rp = c->range;
  IpArgs a{};
  a.Ri = rp.ri_off[s.dhi] - rp.ri_off[s.dlo];
  a.tests = rp.ip_tests.as<DIPTest>() + rp.ri_off[s.dlo];
  a.grp = IP_GROUP;
  a.c0 = s.c0, a.nch = s.nch, a.w0 = s.w0, a.nw = s.nw;
  if (!a.Ri || !s.nch) return a;
  if (c->pb.may_err) {  // k_ip_rows<true>
    // batch size: as many peers per block as keep >= ~2048 blocks in flight, at most IPB_BATCH
    const uint64_t wch = (s.nw + 3) / 4;
    const uint64_t nb_want = (2048 + wch - 1) / wch;
    a.batch = uint32_t(std::max<uint64_t>(1, std::min<uint64_t>(IPB_BATCH, (a.Ri + nb_want - 1) / nb_want)));
    a.nb = nb32(wch * ((a.Ri + a.batch - 1) / a.batch));
  } else if (items && rp.ip_items) {
    a.items = rp.ipi_items.as<DIPItem>() + rp.ipi_off[s.x];
    a.n_items = rp.ipi_off[s.x + 1] - rp.ipi_off[s.x];
    a.ilist = rp.ipi_list.as<uint32_t>();
    a.nb = nb32((uint64_t(a.n_items) + 3) / 4);
  } else {
    a.nb = nb32(uint64_t((a.Ri + a.grp - 1) / a.grp) * ((s.nch + 3) / 4));  // peer groups x blocks of 4 chunks
  }
  return a;
}
static IpRangeArgs ip_range_args(cyc_ctx* c, const PeerSeg& s) {
  RangePlan& rp = c->range;
  IpRangeArgs a{};
  a.Rr = rp.rr_off[s.dhi] - rp.rr_off[s.dlo];
  a.rt = rp.ipr_tests.as<DIPRange>() + rp.rr_off[s.dlo];
  a.iv = rp.ipr_iv.as<uint2>();
  a.sorted = c->prep.ipsort.as<uint32_t>();
  a.c0 = s.c0, a.nch = s.nch;
  a.nb = a.Rr && s.nch ? nb32((uint64_t(a.Rr) + 3) / 4) : 0u;
  return a;
}
static IpIvArgs ip_iv_args(cyc_ctx* c, const PeerSeg& s) {
  RangePlan& rp = c->range;
  IpIvArgs a{};
  a.Rv = rp.rv_off[s.dhi] - rp.rv_off[s.dlo];
  a.rt = rp.ipv_tests.as<DIPIv>() + rp.rv_off[s.dlo];
  a.iv = rp.ipv_iv.as<uint2>();
  a.c0 = s.c0, a.nch = s.nch;
  a.nb = a.Rv && s.nch ? nb32((uint64_t(a.Rv) + 3) / 4) : 0u;
  return a;
}
// identity sets of direction x (IDO builds): its distinct matchers only, the ingress ones over the
// window's identity words
static IdentArgs ident_args(cyc_ctx* c, int x) {
  RangePlan& rp = c->range;
  const uint32_t E = c->prep.dir[1].n, EW = (E + 63) / 64, u0 = rp.rpu_off[x];
  IdentArgs a{};
  a.Ru = rp.rpu_off[x + 1] - u0;
  a.pod_peers = rp.pod_peers_u.as<uint32_t>() + u0;
  a.idob = c->prep.idob.as<uint64_t>() + uint64_t(u0) * EW;
  a.ew0 = x == 0 ? rp.ido_ew0 : 0u;
  a.new_ = x == 0 ? rp.ido_ew1 - rp.ido_ew0 : EW;
  a.grp_ns = rp.ido_grp_ns.as<uint2>() + rp.ido_goff[x];
  a.word_ns = rp.ido_word_ns.as<uint2>();
  a.pbrec = rp.pb_rec.p && CYC_PB_REC ? rp.pb_rec.as<uint4>() + 3 * uint64_t(u0) : nullptr;
  a.nb = a.Ru && E && a.new_ ? nb32((uint64_t((a.Ru + PB_GROUP - 1) / PB_GROUP) * a.new_ + 3) / 4) : 0u;
  return a;
}
// full pod-peer rows, a wave per (PR_DIRECT_G pod peers, word)
static PodDirectArgs pod_direct_args(cyc_ctx* c, const PeerSeg& s) {
  RangePlan& rp = c->range;
  PodDirectArgs a{};
  a.Rp = rp.rp_off[s.dhi] - rp.rp_off[s.dlo];
  a.pod_peers = rp.pod_peers.as<uint32_t>() + rp.rp_off[s.dlo];
  a.w0 = s.w0, a.nw = s.nw;
  a.nb = a.Rp && c->prep.dir[1].n && s.nw ? nb32((uint64_t((a.Rp + PR_DIRECT_G - 1) / PR_DIRECT_G) * s.nw + 3) / 4) : 0u;
  return a;
}
// pod-peer rows through identity outcomes and word runs (k_peer_ident, then k_pod_rows)
static PodRunsArgs pod_runs_args(cyc_ctx* c, const PeerSeg& s) {
  Prepared& prep = c->prep;
  RangePlan& rp = c->range;
  const uint32_t E = prep.dir[1].n, r0 = rp.rp_off[s.dlo];
  PodRunsArgs a{};
  a.Rp = rp.rp_off[s.dhi] - r0;
  a.pod_peers = rp.pod_peers.as<uint32_t>() + r0;
  a.ido = prep.ido.as<uint8_t>() + uint64_t(r0) * E;
  a.word_off = prep.word_off.as<uint32_t>();
  a.run_e = prep.run_e.as<uint32_t>();
  a.run_mask = prep.run_mask.as<uint64_t>();
  a.w0 = s.w0, a.nw = s.nw;
  if (a.Rp && E && s.nw) a.nb_ident = grid1(uint64_t(a.Rp) * E, 256), a.nb = nb32(uint64_t((s.nw + 255) / 256) * a.Rp);
  return a;
}
// PM builds' sparse pod-peer rows and posting-built rows (launch C), grp peers per block
static PodSparseArgs pod_sparse_args(cyc_ctx* c, const PeerSeg& s, uint32_t grp) {
  RangePlan& rp = c->range;
  const uint32_t E = c->prep.dir[1].n;
  const uint64_t cb = (s.nch + 3) / 4;
  PodSparseArgs a{};
  a.Rp = rp.scan_off[s.dhi] - rp.scan_off[s.dlo];
  a.grp = grp;
  a.plist = rp.pp_scan.as<uint32_t>() + rp.scan_off[s.dlo];
  a.plist_post = rp.pp_post.as<uint32_t>() + rp.post_off[s.dlo];
  a.c0 = s.c0, a.nch = s.nch;
  a.nb = a.Rp && E && cb ? nb32((uint64_t(a.Rp) + grp - 1) / grp * cb) : 0u;
  a.nb_post = E && s.nch ? rp.post_off[s.dhi] - rp.post_off[s.dlo] : 0u;  // a block per posting-built peer
  return a;
}

// Pipeline pieces.  Steps 1, 3, 4 are shared; steps 2 and 5-7 run per direction (ingress peers,
// targets, class rows and plane are disjoint from egress ones), so the two directions can run
// as two independent branches: one direction's front hides under the other's HBM-bound emit.
enum { COMMON_SELECTORS = 1, COMMON_PORTS = 2, COMMON_FILL = 4, COMMON_ALL = 7 };

static void enq_common(cyc_ctx* c, hipStream_t st, int parts = COMMON_ALL) {
  if (parts & COMMON_FILL) launch(k_fill_u32, fill_args(c, false), st);
  if (parts & COMMON_SELECTORS) launch(c->prep.dense_sel ? k_selectors_dense : k_selectors, sel_args(c, false), st);
  if (!(parts & COMMON_PORTS)) return;
  launch(k_portok, port_args(c), st);
  launch(k_portbits, port_bits_args(c, c->route, false), st);
  launch(k_slot_words, slot_words_args(c), st);
}

// d = 2: both directions — in one launch (their peer sub-lists are adjacent) when they share a window
enum { PEERS_POD = 1, PEERS_IP = 2 };
static void enq_peer_rows(cyc_ctx* c, int d, hipStream_t st, int which = PEERS_POD | PEERS_IP) {
  const Route& route = c->route;
  const bool err = c->pb.may_err;
  PeerCommon pc = peer_common(c);
  pc.sv.selres = c->prep.selres.as<uint8_t>();  // this path always builds the table (enq_common); its kernels read it
  for (int x = d == 2 ? 0 : d; x < (d == 2 ? 2 : d + 1); x++) {
    const PeerSeg s = peer_seg(c, d == 2 && route.one_window, x);
    if ((which & PEERS_POD) && route.ido) {
      for (int dx = s.dlo; dx < s.dhi; dx++) launch(k_peer_bits, pc, ident_args(c, dx), st);
    } else if ((which & PEERS_POD) && route.pod_direct) {
      launch(err ? k_pod_rows_direct<true> : k_pod_rows_direct<false>, pc, pod_direct_args(c, s), st);
    } else if (which & PEERS_POD) {
      const PodRunsArgs a = pod_runs_args(c, s);
      if (a.nb) k_peer_ident<<<a.nb_ident, 256, 0, st>>>(pc, a);
      launch(err ? k_pod_rows<true> : k_pod_rows<false>, pc, a, st);
    }
    if (!(which & PEERS_IP)) continue;
    launch(k_ip_rows_iv, pc, ip_iv_args(c, s), st);
    launch(k_ip_rows_range, pc, ip_range_args(c, s), st);
    launch(err ? k_ip_rows<true> : k_ip_rows_fast, pc, ip_args(c, s, false), st);
  }
}

// 5. membership + classes of direction d
static void enq_member_clear(cyc_ctx* c, int d, hipStream_t st) {
  DirDev& dd = c->prep.dir[d];
  if (dd.n) HIPCHK(hipMemsetAsync(dd.ht_key.p, 0xFF, dd.ht_key.bytes, st));  // keys and reps: one buffer
}

// The class rows of a run empty the hash table for the next one (ht_clear_slice); only runs whose
// class rows do not launch (no slots or no pods) need the memset (prepare_device empties it once).
static bool class_rows_clear_ht(const cyc_ctx* c, int d) {
  return c->prep.dir[d].n && c->pb.K && c->pb.W && c->range.n_act[d];
}

static void enq_member(cyc_ctx* c, int d, hipStream_t st, bool clear = true) {
  DirDev& dd = c->prep.dir[d];
  if (!dd.n) return;
  if (clear && !class_rows_clear_ht(c, d)) enq_member_clear(c, d, st);
  MemberArgs ma = member_args(c, d);
  if (!c->range.n_act[d]) return;
  if (c->route.member_wave[d]) k_member_wave<<<unsigned((uint64_t(c->range.n_act[d]) + 3) / 4), 256, 0, st>>>(ma);
  else k_member<<<grid1(c->range.n_act[d], 128), 128, 0, st>>>(ma);
  k_classify<<<grid1(c->range.n_act[d], 256), 256, 0, st>>>(ma, dd.class_of.as<uint32_t>());
}

// 6. class rows of direction d
// IDO class rows: representatives per block (cyc_set_option "class_rpb"; 0 = auto: 4, or more in
// the fused front, build_front), as many as fit the staged identity-set budget
static uint32_t class_rpb(const cyc_ctx* c, size_t per_rep_lds, uint32_t want = 0) {
  const uint64_t fit = std::max<uint64_t>(1, IDO_LDS_BYTES / std::max<size_t>(per_rep_lds, 1));
  const int64_t w = want ? int64_t(want) : c->opt.class_rpb ? c->opt.class_rpb : 4;
  return uint32_t(std::max<int64_t>(1, std::min<int64_t>(w, int64_t(fit))));
}
// ... their LDS bytes per representative: set_rows identity sets (KC slot rows, or D descriptor rows)
// + staged IP peers (+ alignment); and their blocks: (256-word group, KC slots, rpb representatives)
static size_t ido_rep_lds(uint32_t set_rows, uint32_t EW) { return size_t(set_rows) * EW * 8 + IDO_IPL * sizeof(uint4) + 16; }
static uint64_t ido_row_blocks(uint32_t WA, uint32_t K, uint32_t KC, uint32_t reps, uint32_t rpb) {
  return uint64_t(ido_chunk_groups(WA)) * ((K + KC - 1) / KC) * ((reps + rpb - 1) / rpb);
}

static RowArgs row_args(cyc_ctx* c, int d) {
  Problem& pb = c->pb;
  Prepared& prep = c->prep;
  RangePlan& rp = c->range;
  const uint32_t P = pb.P, K = pb.K, W = pb.W, D = uint32_t(std::max<size_t>(pb.descs.size(), 1));
  DirDev& dd = prep.dir[d];
  RowArgs ra{};
  ra.tgt = dd.tgt.as<DTarget>();
  ra.peers = prep.peers.as<DPeer>();
  ra.PM = prep.PM.as<uint64_t>();
  ra.ER = prep.ER.as<uint64_t>();
  ra.portok = prep.portok.as<uint8_t>();
  // descriptor bit rows of the port table (k_portbits; computed whenever D <= 32)
  ra.portbits = c->route.port_bits && pb.pms.size() && pb.descs.size() ? prep.portbits.as<uint32_t>() : nullptr;
  ra.D = D;
  ra.n_ident = dd.n;
  ra.K = K;
  ra.W = W;
  ra.P = P;
  peer_window(c->range, c->pb.W, d, ra.w0, ra.WA);  // the class rows cover their peers' word window
  if (!c->pb.blocks.empty()) {     // batched blocks: each class row covers its block's words
    ra.w0 = 0;
    ra.WA = prep.blk_wa_max;
    ra.id_win = prep.id_win[d].as<uint2>();
  }
  ra.class_of = dd.class_of.as<uint32_t>();
  ra.cnt = dd.cnt.as<uint32_t>();
  ra.list_off = dd.list_off.as<uint32_t>();
  ra.list = dd.list.as<uint32_t>();
  ra.id_err = dd.err.as<uint8_t>();
  ra.id_desc = dd.id_desc.as<int32_t>();
  ra.id_status = dd.id_status.as<uint8_t>();
  ra.VALID = prep.VALID.as<uint64_t>();
  ra.DESCW = prep.DESCW.as<int32_t>();
  ra.DM = prep.DM.as<uint64_t>();
  ra.A = dd.A.as<uint64_t>();
  ra.AE = pb.may_err ? dd.AE.as<uint64_t>() : nullptr;
  ra.rep_blocks = rp.n_act[d];  // k_class_rows (panic path): a block row per representative slot
  ra.reps = dd.reps.as<uint32_t>();
  ra.rep_cnt = dd.rep_cnt();
  ra.IDOB = prep.idob.as<uint64_t>();
  ra.peer_ido = rp.peer_ido.as<uint32_t>();
  ra.prow = rp.peer_row.as<uint32_t>();
  ra.zero = prep.zeros.as<uint64_t>();
  ra.runs = prep.runs.as<WordRuns>();
  ra.B = dd.B.as<uint64_t>();
  ra.ip_off = dd.ip_off.as<uint32_t>();
  ra.ip_cnt = dd.ip_cnt.as<uint32_t>();
  ra.ip_list = dd.ip_list.as<uint4>();
  ra.ip_rng = prep.ip_rng.as<uint32_t>();
  ra.ip_cnz = ip_cnz(c);
  ra.E = prep.dir[1].n;
  ra.EW = (ra.E + 63) / 64;
  ra.ew_lo = d == 0 ? rp.ido_ew0 : 0u;
  ra.ew_hi = d == 0 ? rp.ido_ew1 : ra.EW;
  ra.NB = d == 0 ? K : D;
  // the first kernel below empties the hash table for the next run (keys + reps; not the counter)
  ra.ht_clear = reinterpret_cast<uint32_t*>(dd.ht_key.p);
  ra.ht_clear_words = uint64_t(dd.ht_cap) * 4;
  ra.rpb = 1;
  return ra;
}

static void enq_class_rows(cyc_ctx* c, int d, hipStream_t st) {
  Problem& pb = c->pb;
  Prepared& prep = c->prep;
  RangePlan& rp = c->range;
  const uint32_t K = pb.K, W = pb.W, D = uint32_t(std::max<size_t>(pb.descs.size(), 1));
  DirDev& dd = prep.dir[d];
  if (!dd.n || !K || !W || !rp.n_act[d]) return;
  RowArgs ra = row_args(c, d);
  if (!ra.WA) return;
  if (pb.may_err) {  // the ordered walk with panic bits: one block row per identity, 8 slots per thread
    const unsigned g = unsigned(uint64_t((ra.WA + 255) / 256) * ((K + 7) / 8) * ra.rep_blocks);
    if (d == 0) k_class_rows<false><<<g, 256, 0, st>>>(ra);
    else k_class_rows<true><<<g, 256, 0, st>>>(ra);
  } else if (c->route.ido) {
    // identity sets first (one wave per representative and 4 slots / descriptors), then the rows
    const uint64_t waves = uint64_t(rp.n_act[d]) * ((ra.NB + CI_G - 1) / CI_G);
    if (d == 0) k_class_ident<false, CI_G><<<unsigned((waves + 3) / 4), 256, 0, st>>>(ra);
    else k_class_ident<true, CI_G><<<unsigned((waves + 3) / 4), 256, 0, st>>>(ra);
    ra.ht_clear_words = 0;
    const size_t per = ido_rep_lds(d == 0 ? 4u : D, ra.EW);  // (class_rows_ido_blk stages KC = 4 slot rows, or D descriptor rows)
    ra.rpb = class_rpb(c, per);
    const unsigned gi = unsigned(ido_row_blocks(ra.WA, K, 4, rp.n_act[d], ra.rpb));
    if (d == 0) k_class_rows_ido<false, 4><<<gi, 256, per * ra.rpb, st>>>(ra);
    else k_class_rows_ido<true, 4><<<gi, 256, per * ra.rpb, st>>>(ra);
  } else {  // per-class flattened peer lists (the IP word spans are final here)
    const bool wave = c->route.pl_wave;
    if (d == 0 && wave) k_class_rows_pl<false, true><<<pl_blocks(c, d), pl_threads(c), 0, st>>>(ra);
    else if (d == 0) k_class_rows_pl<false, false><<<pl_blocks(c, d), pl_threads(c), 0, st>>>(ra);
    else if (wave) k_class_rows_pl<true, true><<<pl_blocks(c, d), pl_threads(c), 0, st>>>(ra);
    else k_class_rows_pl<true, false><<<pl_blocks(c, d), pl_threads(c), 0, st>>>(ra);
  }
}

// 7. the emit: both planes (ingress rows to out_in, egress rows to out_eg) in one launch — two
// when their rows differ in length (a source shard: ingress rows of every destination over the
// shard's word window, egress rows of its sources over all words).  d_status (may be null): the
// status plane, copied by the (first) emit's blocks.  Returns false if no emit was launched (no rows
// in the plan; the caller then copies the status plane itself).
constexpr uint64_t EMIT_WIDE_MIN = 16384;  // shortest plane row (bytes) emitted a block per row; shorter: k_emit_flat
// k_emit_units over ea.n_rows[] rows of ea.pl_words[] words per plane (16-byte aligned planes, even
// row words): units of about one 1024 x 7 x 16 B block pass (114 KB) — whole rows of up to that, or
// several shorter rows — so a block resolves its rows' order -> identity -> class chains together
static const char* enq_emit_units(EmitArgs ea, hipStream_t st) {
  constexpr uint64_t pass = 1024 * 7 * 16;
  for (int pl = 0; pl < 2; pl++) {
    const uint64_t rb = std::max<uint64_t>(ea.pl_words[pl] * 8, 1);
    ea.unit_rows[pl] = uint32_t(std::min<uint64_t>(EMIT_UNIT_MAX_ROWS, std::max<uint64_t>(1, pass / rb)));
    // rows of 7-14 KB (a source shard's ingress rows at N = 8: 12.5 KB) as 8 rows a unit, a row per
    // 128-thread group in one aligned buffer-op pass: config #3 rank 0 of 8 emit 384 vs 425 us, step
    // -3 %; 512- and 256-thread groups for the 50 / 25 KB rows of N = 2 / 4 measured +1 % / ±0: not
    // used (profiles/r05_row_alignment.txt)
    ea.unit_grp[pl] = 0;
    if (rb <= pass / 8 && rb > pass / 16 && rb % 16 == 0) {
      ea.unit_grp[pl] = 8;
      ea.unit_rows[pl] = 8;
    }
    ea.n_units[pl] = (ea.n_rows[pl] + ea.unit_rows[pl] - 1) / ea.unit_rows[pl];
  }
  ea.per_xcd = (ea.n_units[0] + ea.n_units[1] + 7) / 8;
  k_emit_units<1024, 7><<<ea.per_xcd * 8, 1024, 0, st>>>(ea);
  return "k_emit_units<1024,7>";
}


static const char* enq_emit_launch(const EmitArgs& ea_in, hipStream_t st, uint64_t* out_in, uint64_t* out_eg) {
  EmitArgs ea = ea_in;
  const uint32_t nr = ea.n_rows[0] + ea.n_rows[1];
  ea.per_xcd = (nr + 7) / 8;
  const bool aligned = reinterpret_cast<uintptr_t>(out_in) % 16 == 0 && reinterpret_cast<uintptr_t>(out_eg) % 16 == 0;
  const unsigned g = ea.per_xcd * 8;  // one block per row slot of the 8 XCD segments
  if (ea.row_words % 2 || !aligned) {
    k_emit_words<<<g, 256, 0, st>>>(ea);
    return "k_emit_words";
  }
  const uint64_t row_bytes = ea.row_words * 8;
  // 56-112 KB rows (config #3's 98 KB): 1024 x 7 blocks through buffer ops, one pass.  A 512 x 13
  // one-pass block held 84 VGPRs with flat addresses (config #3 3.5 % slower, profiles/r03_emit_ab.txt)
  // and 54 through buffer ops, 1-2 % ahead of 1024 x 7 on the best plane placements but up to 20 %
  // behind on others: over 14 placements 3.542 vs 3.389 ms per step (profiles/r05_plane_placement.txt;
  // the flat-address 1024 x 7 form trailed both) — only 1024 x 7 through buffer ops is kept.
  // (128 x 13 buffer blocks for config #4's 25 KB rows lost: 442-447 vs 419-424 us.)
  if (row_bytes > 512 * 7 * 16 && row_bytes <= 1024 * 7 * 16) {
    k_emit_wide_buf<1024, 7><<<g, 1024, 0, st>>>(ea);
    return "k_emit_wide_buf<1024,7>";
  } else if (row_bytes > 512 * 7 * 16) {  // > 112 KB (114,688 B): 1024 x 7 passes
    k_emit_wide<1024, 7><<<g, 1024, 0, st>>>(ea);
    return "k_emit_wide<1024,7>";
  } else if (row_bytes > 256 * 8 * 16) {  // 32-56 KB: 512 x 7 (source shards at N = 2)
    k_emit_wide<512, 7><<<g, 512, 0, st>>>(ea);
    return "k_emit_wide<512,7>";
  } else if (row_bytes >= EMIT_WIDE_MIN) {  // 256-thread single pass (16-32 KB rows; buffer-op 256 x 8,
                                            // 512 x 4 and 1024 x 2 blocks were no better over 4 plane
                                            // placements of config #4, profiles/r05_plane_placement.txt)
    const uint64_t need = (ea.row_words / 2 + 255) / 256;  // 4 (EMIT_WIDE_MIN) to 8
    if (need <= 4) k_emit_wide<256, 4><<<g, 256, 0, st>>>(ea);
    else if (need <= 6) k_emit_wide<256, 6><<<g, 256, 0, st>>>(ea);
    else if (need <= 7) k_emit_wide<256, 7><<<g, 256, 0, st>>>(ea);
    else k_emit_wide<256, 8><<<g, 256, 0, st>>>(ea);
    return need <= 4 ? "k_emit_wide<256,4>" : need <= 6 ? "k_emit_wide<256,6>"
         : need <= 7 ? "k_emit_wide<256,7>" : "k_emit_wide<256,8>";
  } else {  // flat multi-row sweep over ~32 KB per block
    ea.chunk = uint32_t(std::min<uint64_t>(EMIT_FLAT_MAX_ROWS, std::max<uint64_t>(1, 32768 / row_bytes)));
    k_emit_flat<256, 8><<<(ea.per_xcd + ea.chunk - 1) / ea.chunk * 8, 256, 0, st>>>(ea);
    return "k_emit_flat<256,8>";
  }
}

static bool enq_emit_blocks(cyc_ctx* c, hipStream_t st, uint64_t* out_in, uint64_t* out_eg, uint8_t* d_status) {
  Problem& pb = c->pb;
  Prepared& prep = c->prep;
  if (pb.blocks.empty()) return false;
  if (!pb.K || !d_status) return true;  // nothing to write (the status plane of blocks is their slabs)
  BlockArgs ba{};
  ba.n_blk = uint32_t(pb.blocks.size());
  ba.K = pb.K;
  ba.AS = prep.blk_wa_max;
  ba.blk = prep.blk.as<uint4>();
  ba.boff = prep.blk_off.as<uint64_t>();
  for (int pl = 0; pl < 2; pl++) {
    ba.pod_id[pl] = prep.dir[pl].pod_id.as<uint32_t>();
    ba.class_of[pl] = prep.dir[pl].class_of.as<uint32_t>();
    ba.A[pl] = prep.dir[pl].A.as<uint64_t>();
  }
  ba.st_src = prep.slot_status.as<uint8_t>();
  ba.out[0] = out_in;
  ba.out[1] = out_eg;
  ba.st_out = d_status;
  // a block's slab words split over workgroups of ~16 words per thread (one workgroup per block
  // left a few large blocks on a few CUs); small blocks' extra workgroups exit at once
  const unsigned bs = prep.blk_np_max * 2 > 128 ? 256 : 128;
  const uint64_t most = 2ull * prep.blk_np_max * pb.K * ((prep.blk_np_max + 63) / 64);  // largest slab, both planes
  ba.split = uint32_t(std::min<uint64_t>(64, std::max<uint64_t>(1, most / (uint64_t(bs) * 16))));
  k_emit_blocks<<<ba.n_blk * ba.split, bs, 0, st>>>(ba);
  return true;
}

// part (row phases): 0 = every row of the plan; 1 / 2 = the rows before / from the split (the plan's
// emit lists hold them in that order); the status plane goes with part 1, the span reset with part 2
// (after the last reader of the IP rows' spans, phase 2's class rows).
static bool enq_emit(cyc_ctx* c, hipStream_t st, uint64_t* out_in, uint64_t* out_eg, uint8_t* d_status, bool inplace = false,
                     int part = 0) {
  Problem& pb = c->pb;
  Prepared& prep = c->prep;
  RangePlan& rp = c->range;
  if (part != 1) prep.ip_rng_clean = false;  // (set again below when this emit resets the spans for the next run)
  const uint32_t K = pb.K;
  const uint64_t rw[2] = {uint64_t(K) * rp.win_wa, uint64_t(K) * pb.W};  // words per plane row
  uint32_t nr[2];
  for (int d = 0; d < 2; d++) nr[d] = rw[d] ? uint32_t(rp.rh[d] - rp.rl[d]) : 0u;
  if (part != 2) {
    c->run.last.emit_kernel.clear();
    c->run.last.emit_launches = 0;
  }
  if (!pb.blocks.empty()) {
    const bool r = enq_emit_blocks(c, st, out_in, out_eg, d_status);
    if (r && pb.K && d_status) c->run.last.emit_kernel = "k_emit_blocks", c->run.last.emit_launches = 1;
    return r;
  }
  if (!nr[0] && !nr[1]) return false;
  EmitArgs ea{};
  ea.st_src = prep.slot_status.as<uint8_t>();
  ea.st_dst = d_status;
  ea.st_bytes = d_status ? uint64_t(pb.P) * K : 0;
  ea.reset = prep.ip_rng.as<uint32_t>();
  ea.reset_n = pb.may_err ? 0u : uint64_t(pb.peers.size()) * 4;  // (k_ip_rows with panics keeps no spans)
  if (part != 1) prep.ip_rng_clean = ea.reset_n != 0;
  for (uint32_t pl = 0; pl < 2; pl++) {
    ea.row_lo[pl] = uint32_t(rp.rl[pl]);
    ea.order[pl] = rp.order[pl].as<uint2>();
    ea.class_of[pl] = prep.dir[pl].class_of.as<uint32_t>();
    ea.A[pl] = prep.dir[pl].A.as<uint64_t>();
    ea.arow[pl] = inplace ? rp.arow[pl].as<uint32_t>() : nullptr;
  }
  ea.out[0] = out_in;
  ea.out[1] = out_eg;
  ea.pl_words[0] = rw[0];
  ea.pl_words[1] = rw[1];
  auto note = [&](const char* k) {  // what cyc_last_emit reports
    std::string& names = c->run.last.emit_kernel;
    if (names.find(k) == std::string::npos) names += (names.empty() ? "" : " + ") + std::string(k);
    c->run.last.emit_launches++;
  };
  if (rw[0] == rw[1] && nr[0] == nr[1]) {  // target rows: both planes in one launch
    ea.row_words = rw[0];
    ea.interleave = c->route.emit_interleave ? 1u : 0u;
    ea.n_rows[0] = ea.n_rows[1] = nr[0];
    if (part) {  // row phases (target rows over the whole table: both planes split at the same row)
      const uint32_t n1 = rp.phase_n1[0];
      ea.n_rows[0] = ea.n_rows[1] = part == 1 ? n1 : nr[0] - n1;
      for (int pl = 0; pl < 2; pl++) ea.order[pl] += part == 1 ? 0u : n1;
      if (part == 1) ea.reset_n = 0;
      else ea.st_bytes = 0;
    }
    note(enq_emit_launch(ea, st, out_in, out_eg));
    return true;
  }
  // rows of different lengths (a source shard): ONE launch over units of about one block pass each
  const bool aligned = reinterpret_cast<uintptr_t>(out_in) % 16 == 0 && reinterpret_cast<uintptr_t>(out_eg) % 16 == 0;
  if (aligned && rw[0] % 2 == 0 && rw[1] % 2 == 0) {
    ea.n_rows[0] = nr[0];
    ea.n_rows[1] = nr[1];
    note(enq_emit_units(ea, st));
    return true;
  }
  bool first = true;
  for (int pl = 0; pl < 2; pl++) {  // (8-byte row words or unaligned planes) one launch per plane
    if (!nr[pl]) continue;
    EmitArgs e1 = ea;
    e1.n_rows[0] = pl == 0 ? nr[0] : 0u;  // the row list is [plane 0 rows][plane 1 rows]
    e1.n_rows[1] = pl == 1 ? nr[1] : 0u;
    e1.row_words = rw[pl];
    if (!first) e1.st_bytes = e1.reset_n = 0;
    first = false;
    note(enq_emit_launch(e1, st, pl == 0 ? out_in : reinterpret_cast<uint64_t*>(16), pl == 1 ? out_eg : reinterpret_cast<uint64_t*>(16)));
  }
  return true;
}

// The fused front (k_front_a..e, one stream): the same block ranges the two-branch DAG launches
// as ~15 kernels (enq_common, enq_peer_rows, enq_member, enq_class_rows), grouped by dependency
// level (Route::fused says where it applies).  build_front sizes it, launch_front issues it.
struct FrontLaunches {
  FrontA fa;
  FrontB fb;
  FrontC fc;
  FrontRows fd, fe;
  uint32_t nd[3][2], ne[3][2];         // blocks of launches D and E per direction: [0] one pass, [1] / [2] a row phase's
  size_t lds = 0, lds_uni = 0;         // launch E's LDS bytes (egress with one descriptor per slot: lds_uni)
  uint32_t* span_fill = nullptr;       // the IP rows' word spans, set to ~0 by a memset before the launches
  size_t span_fill_bytes = 0;          // (0: the previous run's emit reset them, or launch A does)
  bool phases = false;
  bool fits = true;                    // every range below 2^30 blocks, every launch below 2^31 (else the DAG path runs)
};

// Host arithmetic only: changes no context state and enqueues nothing.
// out_in / out_eg non-null: the class rows go straight into those planes (in-place class rows; the
// emit must then be enqueued with inplace = true).
// phases (row phases, Route::phase_split): the class rows as two launches, phase 1's emit between them.
static FrontLaunches build_front(cyc_ctx* c, const Route& route, uint64_t* out_in, uint64_t* out_eg, bool phases) {
  Problem& pb = c->pb;
  Prepared& prep = c->prep;
  RangePlan& rp = c->range;
  const uint32_t K = pb.K, D = uint32_t(std::max<size_t>(pb.descs.size(), 1));
  FrontLaunches fl{};
  fl.phases = phases;
  bool& fits = fl.fits;
  auto blocks = [&fits](uint64_t n) {
    fits = fits && n < (1ull << 30);
    return uint32_t(n);
  };
  FrontA& fa = fl.fa;
  FrontB& fb = fl.fb;
  FrontC& fc = fl.fc;
  FrontRows &fd = fl.fd, &fe = fl.fe;
  const bool ido = route.ido;
  // A: IP word spans | port table | slot words | selectors
  const FillArgs fill = fill_args(c, !ido && rp.Rp);
  const PortArgs ports = port_args(c);
  SlotWordsArgs slots = slot_words_args(c);
  if (!route.slot_words) slots.nb = 0;
  fa.sel = sel_args(c, route.lazy_sel);
  // B: IP rows | pod-peer identity sets (both directions' adjacent sub-lists) | membership x 2
  fb.pc = peer_common(c);
  uint32_t pr_grp = 0;
  if (!ido && route.pod_sparse) {
    // a wave per chunk over groups of 8 peers once that fills the chip (>= 64k peer chunks:
    // config #3u 2.6 vs 3.2 ms), else the 4 waves of a block share each chunk (config #2)
    uint64_t peer_chunks_all = 0;
    for (int x = 0; x < 2; x++) {
      const PeerSeg s = peer_seg(c, route.one_window, x);
      peer_chunks_all += uint64_t(rp.scan_off[s.dhi] - rp.scan_off[s.dlo]) * s.nch;
    }
    pr_grp = c->opt.pr_group > 0 ? uint32_t(c->opt.pr_group) : (peer_chunks_all >= 65536 ? 8u : 1u);
    fc.pc = fb.pc;
  }
  for (int x = 0; x < 2; x++) {
    const PeerSeg s = peer_seg(c, route.one_window, x);
    fb.ip[x] = ip_args(c, s, true);
    fb.ip_range[x] = ip_range_args(c, s);
    fb.ip_iv[x] = ip_iv_args(c, s);
    if (ido) fb.ident[x] = ident_args(c, x);
    // PM builds, few pod-peer words: full rows, a wave per (pod peer, word); else sparse pod-peer rows
    // in launch C (k_front_c)
    else if (!route.pod_sparse) fb.pods[x] = pod_direct_args(c, s);
    else fc.pods[x] = pod_sparse_args(c, s, pr_grp);
  }
  size_t &lds = fl.lds, &lds_uni = fl.lds_uni, e_per[2] = {0, 0};
  uint32_t na_all[2];  // active identities per direction
  for (int d = 0; d < 2; d++) {
    const uint32_t na = na_all[d] = prep.dir[d].n ? rp.n_act[d] : 0u;
    fb.member[d].a = fc.elect[d].a = member_args(c, d);
    if (phases) {  // the class election lists phase 2's classes apart (from the tail of reps[])
      fc.elect[d].a.first_row = rp.arow[d].as<uint32_t>();
      fc.elect[d].a.split = route.phase_split;
    }
    fc.elect[d].class_of = prep.dir[d].class_of.as<uint32_t>();
    fb.member[d].wave = route.member_wave[d];
    fb.member[d].nb = nb32(fb.member[d].wave ? (uint64_t(na) + 3) / 4 : (uint64_t(na) + 255) / 256);
    fc.elect[d].nb = nb32((uint64_t(na) + 255) / 256);
    if (!na) continue;
    fd.ra[d] = row_args(c, d);  // its blocks empty the direction's hash table for the next run
    if (out_in && out_eg) {
      fd.ra[d].A = d == 0 ? out_in : out_eg;
      fd.ra[d].arow = rp.arow[d].as<uint32_t>();
    }
    // (the class election keeps a launch of its own, C: electing inside the next launch's blocks put
    // the election chain on every block — IDO identity sets C + D 29 -> 45 us, PM class rows C + D
    // 79 -> 117 us on config #4: profiles/r04_elect_ab.txt)
    if (!ido) {  // PM builds: launch D (k_front_d_pm) is the class rows from flattened peer lists
      fd.nb(d) = pl_blocks(c, d);
      if (d == 1 && prep.uni_desc && c->pb.blocks.empty()) fd.ra[d].udesc = prep.udesc.as<int32_t>();
      fd.ra[d].pod_sparse = route.pod_sparse;  // pod rows from pod_rows_sparse_blk (launch C)
      continue;
    }
    fe.ra[d] = fd.ra[d];
    fe.ra[d].ht_clear_words = 0;  // (launch D's identity sets empty it)
    fd.nb(d) = blocks((uint64_t(na) * ((fd.ra[d].NB + CI_G - 1) / CI_G) + 3) / 4);
    // egress with one descriptor per slot (udesc): only the block's slots' sets are staged
    if (d == 1 && prep.uni_desc) fe.ra[d].udesc = prep.udesc.as<int32_t>();
    e_per[d] = ido_rep_lds(d == 0 || fe.ra[d].udesc ? uint32_t(E_KC) : D, fd.ra[d].EW);
  }
  // launch E's representatives per block: the most of 16 / 8 that still leaves >= 3000 blocks
  // (about two rounds of the chip's resident blocks: one block's staging latency is paid once per
  // 16 representatives), else 4 (config #3: E 106 -> 96 us at N = 1 with 16; at N = 8 a source
  // shard's ~1,900 blocks of 4 ran 22.8 us, of 8 24.0 — profiles/r04_class_rpb_ab.txt).  With row
  // phases each of the two launches computes about half of the classes, so half of its blocks count
  // (config #3 phased E per step, 8 per block against 16: 121.4 vs 141.8 us on one box, 122.8 vs 123.8
  // on another — profiles/r06_class_rpb_ab.txt)
  auto e_blocks = [&](int d, uint32_t rpb) { return ido_row_blocks(fe.ra[d].WA, K, E_KC, na_all[d], rpb); };
  uint32_t e_want = uint32_t(c->opt.class_rpb);
  if (!e_want) {
    e_want = 4;
    for (uint32_t cand : {16u, 8u}) {
      uint64_t tot = 0;
      for (int d = 0; d < 2; d++)
        if (e_per[d]) tot += e_blocks(d, class_rpb(c, e_per[d], cand));
      if ((phases ? tot / 2 : tot) >= 3000) {
        e_want = cand;
        break;
      }
    }
  }
  for (int d = 0; d < 2; d++) {
    if (!e_per[d]) continue;
    fe.ra[d].rpb = class_rpb(c, e_per[d], e_want);
    fe.nb(d) = blocks(e_blocks(d, fe.ra[d].rpb));
    if (d == 1 && fe.ra[d].udesc) lds_uni = e_per[d] * fe.ra[d].rpb;
    else lds = std::max<size_t>(lds, e_per[d] * fe.ra[d].rpb);
  }
  // membership ahead of the rest of launch B unless the IP rows alone fill the chip (~2k resident blocks)
  fb.member_first = uint64_t(fb.ip[0].nb) + fb.ip[1].nb < 2048;
  // Without a selector table to build (lazy selectors) launch A is dropped: its port table, slot
  // words and port bits (from the matchers directly) join launch B — their readers are the class
  // rows, launches D / E — and the IP rows' word spans were reset by the previous run's emit
  // (EmitArgs::reset; a memset when they were not).  Captured graphs keep launch A: a replay must not
  // depend on the step before it.
  const bool drop_a = fa.sel.nb == 0 && !c->run.capturing;
  fb.port_bits = port_bits_args(c, route, drop_a);
  fe.ra[1].portbits = fb.port_bits.nb && fe.nb_eg ? prep.portbits.as<uint32_t>() : nullptr;
  if (drop_a) {
    fb.port_table = ports, fb.slot_words = slots;
    if (fill.n && !prep.ip_rng_clean) fl.span_fill = fill.p, fl.span_fill_bytes = fill.n * 4;
  } else {
    fa.fill = fill, fa.port_table = ports, fa.slot_words = slots;
  }
  // the class rows' grids: one pass, or per row phase only the identities that can represent the
  // phase's classes (the representatives' first rows decide the phase), not every active identity
  for (uint32_t phase = 0; phase < 3; phase++)
    for (int d = 0; d < 2; d++) {
      fl.nd[phase][d] = fd.nb(d);
      fl.ne[phase][d] = fe.nb(d);
      if (!CYC_PHASE_GRID || !phase) continue;
      const uint32_t nph = phase == 1 ? rp.n_act_ph1[d] : na_all[d] - rp.n_act_ph1[d];
      if (ido && fe.nb(d)) fl.ne[phase][d] = blocks(ido_row_blocks(fe.ra[d].WA, K, E_KC, nph, fe.ra[d].rpb));
      else if (!ido && fd.nb(d)) fl.nd[phase][d] = std::min(fd.nb(d), nph);
    }
  // (a range of >= 2^30 blocks counts NB_OVER: its launch then fails the sum)
  fits = fits && fa.blocks() < (1ull << 31) && fb.blocks() < (1ull << 31) && fc.blocks() < (1ull << 31);
  return fl;
}

// The events an eager run records for its phase timings (graph / eager-DAG runs: none)
struct FrontEvents {
  hipEvent_t front = nullptr, rows = nullptr;  // after launches A-C; after the (first phase's) class rows
  hipEvent_t mid0 = nullptr, mid1 = nullptr;   // around phase 2's class rows
};

// Issues what build_front sized.  mid (row phases): enqueues phase 1's emit between the two class-row launches.
template <class Mid>
static void launch_front(cyc_ctx* c, hipStream_t st, FrontLaunches& fl, const FrontEvents& ev, const Mid& mid) {
  FrontRows &fd = fl.fd, &fe = fl.fe;
  const bool ido = c->route.ido;
  if (fl.span_fill) HIPCHK(hipMemsetAsync(fl.span_fill, 0xFF, fl.span_fill_bytes, st));
  if (fl.fa.blocks()) k_front_a<<<unsigned(fl.fa.blocks()), 256, 0, st>>>(fl.fa);
  if (fl.fb.blocks()) k_front_b<<<unsigned(fl.fb.blocks()), 256, 0, st>>>(fl.fb);
  if (fl.fc.blocks()) k_front_c<<<unsigned(fl.fc.blocks()), 256, 0, st>>>(fl.fc);
  if (ev.front) HIPCHK(hipEventRecord(ev.front, st));  // eager runs: phase timings
  if (ido && fd.nb_in + fd.nb_eg) k_front_d<<<fd.nb_in + fd.nb_eg, 256, 0, st>>>(fd);  // identity sets: once
  // the class rows: once, or per row phase with phase 1's emit between (mid)
  auto class_rows = [&](uint32_t phase) {
    for (int d = 0; d < 2; d++) {
      (ido ? fe : fd).ra[d].phase = phase;
      fd.nb(d) = fl.nd[phase][d];
      fe.nb(d) = fl.ne[phase][d];
    }
    const size_t lds = fl.lds, lds_uni = fl.lds_uni;
    if (!ido) {
      const unsigned gd = fd.nb_in + fd.nb_eg;
      if (gd && c->route.pl_wave) k_front_d_pm<true><<<gd, pl_threads(c), 0, st>>>(fd);
      else if (gd) k_front_d_pm<false><<<gd, pl_threads(c), 0, st>>>(fd);
    } else if (fe.nb_in && fe.nb_eg && fe.ra[1].udesc) {
      k_front_e_uni<<<fe.nb_in + fe.nb_eg, 256, std::max(lds, lds_uni), st>>>(fe);
    } else {  // the directions' class rows as two launches, each at its own register budget (egress 101
              // VGPRs, ingress 61: one launch at 101 ran config #3 189 -> 170 us, profiles/r03_e_split_ab.txt)
      if (fe.nb_eg && fe.ra[1].udesc) k_class_rows_ido<true, E_KC, true><<<fe.nb_eg, 256, lds_uni, st>>>(fe.ra[1]);
      else if (fe.nb_eg) k_class_rows_ido<true, E_KC><<<fe.nb_eg, 256, lds, st>>>(fe.ra[1]);
      if (fe.nb_in) k_class_rows_ido<false, E_KC><<<fe.nb_in, 256, lds, st>>>(fe.ra[0]);
    }
  };
  class_rows(fl.phases ? 1u : 0u);
  if (ev.rows) HIPCHK(hipEventRecord(ev.rows, st));
  if (fl.phases) {
    mid();
    if (ev.mid0) HIPCHK(hipEventRecord(ev.mid0, st));
    class_rows(2u);
    if (ev.mid1) HIPCHK(hipEventRecord(ev.mid1, st));
  }
}

// The skeleton enqueue_pipeline and capture_pipeline share: the in-place decision, the fused front and its
// emit (row phases: part 1 between the class-row launches, then part 2).  Returns false with nothing
// enqueued and phase_used == 0 when the front is not fused (the caller's fallback runs); else
// *status_done = the emit wrote the status plane.
static bool enq_fused_step(cyc_ctx* c, hipStream_t st, uint64_t* d_in, uint64_t* d_eg, uint8_t* d_status, const FrontEvents& ev,
                           bool* status_done) {
  const Route& route = c->route;
  c->run.last.phase_used = 0;
  if (!route.fused) return false;
  const bool ip = route.inplace && d_in && d_eg;
  const bool phases = route.phase_split != 0;
  FrontLaunches fl = build_front(c, route, ip ? d_in : nullptr, ip ? d_eg : nullptr, phases);
  if (!fl.fits) return false;
  if (phases) c->run.last.phase_used = 2;
  launch_front(c, st, fl, ev, [&] { enq_emit(c, st, d_in, d_eg, d_status, ip, 1); });
  *status_done = enq_emit(c, st, d_in, d_eg, d_status, ip, phases ? 2 : 0);
  return true;
}

// Eager launch, in phase order with the timing events: [0] start, [1] after the front (peer
// rows, classes), [2] after the class rows, [3] after both emits.
static void enqueue_pipeline(cyc_ctx* c, hipStream_t st, uint64_t* d_in, uint64_t* d_eg, uint8_t* d_status) {
  Problem& pb = c->pb;
  Prepared& prep = c->prep;
  RunState& run = c->run;
  HIPCHK(hipEventRecord(run.ev[0], st));
  bool status_done = false;
  if (!enq_fused_step(c, st, d_in, d_eg, d_status, FrontEvents{run.ev[1], run.ev[2], run.ev_p[0], run.ev_p[1]}, &status_done)) {
    enq_common(c, st);
    for (int d = 0; d < 2; d++) enq_peer_rows(c, d, st);
    for (int d = 0; d < 2; d++) enq_member(c, d, st);
    HIPCHK(hipEventRecord(run.ev[1], st));
    for (int d = 0; d < 2; d++) enq_class_rows(c, d, st);
    HIPCHK(hipEventRecord(run.ev[2], st));
    status_done = enq_emit(c, st, d_in, d_eg, d_status);
  }
  HIPCHK(hipEventRecord(run.ev[3], st));
  if (!status_done && d_status && uint64_t(pb.P) * pb.K)
    HIPCHK(hipMemcpyAsync(d_status, prep.slot_status.p, uint64_t(pb.P) * pb.K, hipMemcpyDeviceToDevice, st));
}

// Graph capture / eager DAG: the fused front on st when it applies; else the two-branch DAG:
// [st3] IP rows of both directions + port tables || [st] selectors, then per direction (ingress on
// st, egress on st2) pod-peer sets -> membership / classes -> (wait for st3) class rows, joined
// into one emit of both planes (fork / join through events, graph dependencies when captured).
static void capture_pipeline(cyc_ctx* c, hipStream_t st, hipStream_t st2, hipStream_t st3, uint64_t* d_in, uint64_t* d_eg,
                             uint8_t* d_status) {
  Problem& pb = c->pb;
  Prepared& prep = c->prep;
  bool status_done = false;
  if (enq_fused_step(c, st, d_in, d_eg, d_status, FrontEvents{}, &status_done)) {
    if (status_done) return;
  } else {
    HIPCHK(hipEventRecord(c->run.fork_ev, st));
    HIPCHK(hipStreamWaitEvent(st3, c->run.fork_ev, 0));
    enq_common(c, st3, COMMON_FILL | COMMON_PORTS);
    enq_peer_rows(c, 2, st3, PEERS_IP);  // both directions' IP rows in one launch
    HIPCHK(hipEventRecord(c->run.ports_ev, st3));
    enq_common(c, st, COMMON_SELECTORS);
    HIPCHK(hipEventRecord(c->run.sel_ev, st));
    HIPCHK(hipStreamWaitEvent(st2, c->run.sel_ev, 0));
    for (int d = 1; d >= 0; d--) {
      hipStream_t s = d ? st2 : st;
      enq_peer_rows(c, d, s, PEERS_POD);
      enq_member(c, d, s);
      HIPCHK(hipStreamWaitEvent(s, c->run.ports_ev, 0));
      enq_class_rows(c, d, s);
    }
    HIPCHK(hipEventRecord(c->run.join_ev, st2));
    HIPCHK(hipStreamWaitEvent(st, c->run.join_ev, 0));
    // the emit also writes the status plane; the copy node below only ends steps without rows
    if (enq_emit(c, st, d_in, d_eg, d_status)) return;
  }
  // The step always ends with the status-plane copy (into a sink buffer when the caller passed no
  // status pointer), so every captured graph has the same shape: one node after the join.
  const uint64_t nst = uint64_t(pb.P) * pb.K;
  uint8_t* dst = d_status && nst ? d_status : prep.status_sink.as<uint8_t>();  // sink: >= 16 B (prepare_device)
  HIPCHK(hipMemcpyAsync(dst, prep.slot_status.p, std::max<uint64_t>(nst, 1), hipMemcpyDeviceToDevice, st));
}

// Destroy the retired execs whose last launch has completed (all of them when `wait`).
static void reap_graphs(cyc_ctx* c, bool wait) {
  size_t keep = 0;
  for (size_t i = 0; i < c->run.retired.size(); i++) {
    RunState::Retired& r = c->run.retired[i];
    if (r.done && wait) (void)hipEventSynchronize(r.done);
    const bool done = !r.done || wait || hipEventQuery(r.done) != hipErrorNotReady;
    if (!done) {
      c->run.retired[keep++] = r;
      continue;
    }
    (void)hipGraphExecDestroy(r.exec);
    if (r.graph) (void)hipGraphDestroy(r.graph);
    if (r.done) (void)hipEventDestroy(r.done);
  }
  c->run.retired.resize(keep);
}

static void drop_graph(cyc_ctx* c) {
  if (c->run.graph_exec) c->run.retired.push_back({c->run.graph_exec, c->run.graph, c->run.graph_done});
  c->run.graph_exec = nullptr;
  c->run.graph = nullptr;
  c->run.graph_done = nullptr;
  reap_graphs(c, false);
}

static void ensure_cap_streams(cyc_ctx* c) {
  if (c->run.cap_stream) return;
  HIPCHK(hipStreamCreateWithFlags(&c->run.cap_stream, hipStreamNonBlocking));
  HIPCHK(hipStreamCreateWithFlags(&c->run.cap_stream2, hipStreamNonBlocking));
  HIPCHK(hipStreamCreateWithFlags(&c->run.cap_stream3, hipStreamNonBlocking));
  HIPCHK(hipEventCreateWithFlags(&c->run.sel_ev, EV_SYNC));
  HIPCHK(hipEventCreateWithFlags(&c->run.ports_ev, EV_SYNC));
  HIPCHK(hipEventCreateWithFlags(&c->run.fork_ev, EV_SYNC));
  HIPCHK(hipEventCreateWithFlags(&c->run.join_ev, EV_SYNC));
}

// Batched blocks: each block's status, as its stand-alone run would end — the job expansion's
// panic, else its first panicking job (its own job order), else its table build's duplicate key —
// into c->run.last.blk_rc / c->run.last.blk_msg.  Synchronises only when the inputs can panic.
static int blocks_status(cyc_ctx* c, hipStream_t st) {
  Problem& pb = c->pb;
  Prepared& prep = c->prep;
  const size_t nb = pb.blocks.size();
  c->run.last.blk_rc.assign(nb, CYC_OK);
  c->run.last.blk_msg.assign(nb, "");
  std::vector<unsigned long long> first(nb, ~0ull);
  if (pb.may_err && pb.P && pb.K) {
    HIPCHK(hipMemsetAsync(prep.first_blk.p, 0xFF, nb * 8, st));
    BlockErrArgs e{};
    e.n_blk = uint32_t(nb);
    e.P = pb.P;
    e.K = pb.K;
    e.AS = prep.blk_wa_max;
    e.blk = prep.blk.as<uint4>();
    e.pod_blk = nullptr;
    e.slot_idx = prep.slot_idx.as<uint32_t>();
    e.slot_status = prep.slot_status.as<uint8_t>();
    e.pod_iid = prep.dir[0].pod_id.as<uint32_t>();
    e.pod_eid = prep.dir[1].pod_id.as<uint32_t>();
    e.class_in = prep.dir[0].class_of.as<uint32_t>();
    e.class_eg = prep.dir[1].class_of.as<uint32_t>();
    e.err_in = prep.dir[0].err.as<uint8_t>();
    e.err_eg = prep.dir[1].err.as<uint8_t>();
    e.AE_in = prep.dir[0].AE.as<uint64_t>();
    e.AE_eg = prep.dir[1].AE.as<uint64_t>();
    e.first = prep.first_blk.as<unsigned long long>();
    e.dchunks = (prep.blk_np_max + 255) / 256;
    DevBuf pod_blk;
    upload(pod_blk, pb.pod_blk);
    e.pod_blk = pod_blk.as<uint32_t>();
    if (prep.dir[0].n && prep.dir[1].n)
      k_first_error_blocks<<<grid1(uint64_t(pb.P) * e.dchunks, 1), 256, 0, st>>>(e);
    HIPCHK(hipMemcpyAsync(first.data(), prep.first_blk.p, nb * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
  }
  const std::string saved = c->err;
  for (size_t b = 0; b < nb; b++) {
    const ProbeBlock& x = pb.blocks[b];
    if (pb.blk_expand_panic[b]) {
      c->run.last.blk_rc[b] = CYC_ERR_PANIC_RUNTIME;
      c->run.last.blk_msg[b] = "runtime error: index out of range [0] with length 0";
    } else if (first[b] != ~0ull) {
      const uint32_t np = x.p1 - x.p0, idx = uint32_t(first[b] % 65536);
      const uint64_t rest = first[b] / 65536;
      c->run.last.blk_rc[b] = describe_panic(c, x.p0 + uint32_t(rest / np), x.p0 + uint32_t(rest % np), x.cfg, idx);
      c->run.last.blk_msg[b] = c->err;
    } else if (!pb.blk_dup_msg[b].empty()) {
      c->run.last.blk_rc[b] = CYC_ERR_DUPLICATE_KEY;
      c->run.last.blk_msg[b] = pb.blk_dup_msg[b];
    }
  }
  c->err = saved;
  return (int)CYC_OK;
}

// allow_capture = false: never capture a graph for this run (cyc_table_run's planes are new on
// every call, so a captured graph would be re-instantiated each time): graphs = 1 runs as 2.
// src: rows [lo, hi) are a source shard (CYC_ROWS_SOURCE), else target rows.
static int run_pipeline(cyc_ctx* c, hipStream_t st, uint64_t* d_in, uint64_t* d_eg, uint8_t* d_status, int64_t lo,
                        int64_t hi, bool allow_capture = true, bool src = false) {
  Problem& pb = c->pb;
  Prepared& prep = c->prep;
  RangePlan& rp = c->range;
  const uint32_t P = pb.P, K = pb.K, W = pb.W;
  if (lo < 0 || hi > int64_t(P) || lo > hi) return fail(c, CYC_ERR_ARG, "row range out of bounds");
  if (src && (lo % 64 || (hi % 64 && hi != int64_t(P))))
    return fail(c, CYC_ERR_ARG, "source rows: row_lo must be a multiple of 64, row_hi too unless it is the pod count");
  if (!rp.is(lo, hi, src)) drop_graph(c);  // range plan buffers are re-made
  ensure_range(c, lo, hi, src);
  const Route& route = c->route;
  if (!prep.plvt_ready && route.fused && route.pod_sparse) {
    drop_graph(c);  // a graph captured without the per-pod table would keep the slower gathers
    ensure_plvt(c, st);
  }
  const bool dag = route.launch == 2 || !allow_capture;  // (of the runs that are not eager)
  if (route.runs_eager) {
    enqueue_pipeline(c, st, d_in, d_eg, d_status);
    c->run.last.timed = true;
    c->run.last.timed_graph = false;
  } else if (dag) {
    // the graph's DAG, enqueued directly: the caller's stream forks to two internal streams and
    // joins them back before the emit (events), without hipGraphLaunch's per-replay latency
    ensure_cap_streams(c);
    if (c->opt.step_events) HIPCHK(hipEventRecord(c->run.ev[0], st));
    capture_pipeline(c, st, c->run.cap_stream2, c->run.cap_stream3, d_in, d_eg, d_status);
    if (c->opt.step_events) HIPCHK(hipEventRecord(c->run.ev[3], st));
    c->run.last.timed = c->opt.step_events != 0;
    c->run.last.timed_graph = true;
  } else {
    // The whole pipeline as one hipGraph (captured once per output buffers / row range):
    // removes the host launch cost of ~16 launches per run (dominant on small problems).
    const void* key[6] = {d_in, d_eg, d_status, reinterpret_cast<void*>(lo), reinterpret_cast<void*>(hi),
                          reinterpret_cast<void*>(intptr_t(src))};
    if (!c->run.graph_exec || memcmp(key, c->run.graph_key, sizeof(key)) != 0) {
      drop_graph(c);
      ensure_cap_streams(c);
      hipGraph_t g = nullptr;
      HIPCHK(hipStreamBeginCapture(c->run.cap_stream, hipStreamCaptureModeThreadLocal));
      c->run.capturing = true;
      try {
        capture_pipeline(c, c->run.cap_stream, c->run.cap_stream2, c->run.cap_stream3, d_in, d_eg, d_status);
      } catch (...) {
        c->run.capturing = false;
        throw;
      }
      c->run.capturing = false;
      HIPCHK(hipStreamEndCapture(c->run.cap_stream, &g));
      c->run.graph = g;  // destroyed with the exec (drop_graph / reap_graphs)
      HIPCHK(hipGraphInstantiate(&c->run.graph_exec, g, nullptr, nullptr, 0));
      HIPCHK(hipEventCreateWithFlags(&c->run.graph_done, EV_SYNC));
      memcpy(c->run.graph_key, key, sizeof(key));
    }
    if (c->opt.step_events) HIPCHK(hipEventRecord(c->run.ev[0], st));
    HIPCHK(hipGraphLaunch(c->run.graph_exec, st));
    HIPCHK(hipEventRecord(c->run.graph_done, st));  // the exec may be retired once this completes
    if (c->opt.step_events) HIPCHK(hipEventRecord(c->run.ev[3], st));
    c->run.last.timed = c->opt.step_events != 0;
    c->run.last.timed_graph = true;
  }
  c->run.last.ran = true;
  c->run.last.stream = st;  // cyc_last_classes waits for this stream only

  if (!pb.blocks.empty()) return blocks_status(c, st);

  // 8. panic path: the first panicking job in job order, as the reference would hit it.  Configs
  // run in order (one RunProbeForConfig each); within one, the job expansion (may panic on a pod
  // without containers) precedes the evaluation, which precedes the table build (duplicate keys).
  uint32_t eval_cfg = pb.n_cfg, eval_s = 0, eval_d = 0, eval_idx = 0;
  if (pb.may_err) {
    if (P >= (1u << 24) || K > 65536)  // k_first_error's job-order key: (s*P + d)*65536 + idx < 2^64
      throw Panic{CYC_ERR_ARG, "inputs that can panic are limited to 2^24 pods and 65536 job slots"};
    HIPCHK(hipMemsetAsync(prep.first_err.p, 0xFF, uint64_t(pb.n_cfg) * 8, st));
    ErrArgs e{};
    e.P = P;
    e.K = K;
    e.W = W;
    e.n_cfg = pb.n_cfg;
    e.row_lo = uint32_t(lo);
    e.row_hi = uint32_t(hi);
    e.src = src ? 1u : 0u;
    e.w0 = rp.win_w0;
    e.WA = rp.win_wa;
    e.slot_status = prep.slot_status.as<uint8_t>();
    e.slot_cfg = prep.slot_cfg.as<uint32_t>();
    e.slot_idx = prep.slot_idx.as<uint32_t>();
    e.pod_iid = prep.dir[0].pod_id.as<uint32_t>();
    e.pod_eid = prep.dir[1].pod_id.as<uint32_t>();
    e.class_in = prep.dir[0].class_of.as<uint32_t>();
    e.class_eg = prep.dir[1].class_of.as<uint32_t>();
    e.err_in = prep.dir[0].err.as<uint8_t>();
    e.err_eg = prep.dir[1].err.as<uint8_t>();
    e.AE_in = prep.dir[0].n ? prep.dir[0].AE.as<uint64_t>() : nullptr;
    e.AE_eg = prep.dir[1].n ? prep.dir[1].AE.as<uint64_t>() : nullptr;
    e.first = prep.first_err.as<unsigned long long>();
    if (P && K) k_first_error<<<grid1(uint64_t((P + 255) / 256) * P, 1), 256, 0, st>>>(e);
    std::vector<unsigned long long> first(std::max<uint32_t>(pb.n_cfg, 1), ~0ull);
    HIPCHK(hipMemcpyAsync(first.data(), prep.first_err.p, uint64_t(pb.n_cfg) * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (uint32_t cc = 0; cc < pb.n_cfg; cc++)
      if (first[cc] != ~0ull) {
        eval_cfg = cc;
        eval_idx = uint32_t(first[cc] % 65536);
        const uint64_t rest = first[cc] / 65536;
        eval_d = uint32_t(rest % P);
        eval_s = uint32_t(rest / P);
        break;
      }
  }
  for (uint32_t cc = 0; cc < pb.n_cfg; cc++) {
    if (pb.expand_panic[cc]) return fail(c, CYC_ERR_PANIC_RUNTIME, "runtime error: index out of range [0] with length 0");
    if (cc == eval_cfg) return describe_panic(c, eval_s, eval_d, eval_cfg, eval_idx);
    if (!pb.dup_key_msg[cc].empty()) return fail(c, CYC_ERR_DUPLICATE_KEY, pb.dup_key_msg[cc]);
  }
  return (int)CYC_OK;
}

// Host-side formatting of the panic message for the identified first panicking job.  The
// device found WHICH job panics; this re-derives the reference's message text for it by
// replaying that single job's evaluation order over the compiled tables (error path only).
int describe_panic(cyc_ctx* c, uint32_t s, uint32_t d, uint32_t cfg, uint32_t idx) {
  Problem& pb = c->pb;
  Prepared& prep = c->prep;
  RangePlan& rp = c->range;
  uint32_t k = 0;
  for (uint32_t kk = 0; kk < pb.K; kk++)
    if (pb.slot_cfg[kk] == cfg && pb.slot_idx[kk] == idx) k = kk;
  std::vector<uint8_t> selres(size_t(pb.S) * pb.L);
  HIPCHK(hipMemcpy(selres.data(), prep.selres.p, selres.size(), hipMemcpyDeviceToHost));
  auto sel = [&](uint32_t sid, uint32_t ls) { return selres[size_t(sid) * pb.L + ls]; };
  auto ip_err = [&](const DPeer& pr, uint32_t q, std::string& msg) -> int {
    const DIPBlock& b = pb.ipbs[pr.ipb];
    auto cidr_msg = [&](uint32_t id) {
      return "unable to parse CIDR '" + pb.cidr_str[id] + "': invalid CIDR address: " + pb.cidr_str[id];
    };
    if (!pb.cidrs[b.cidr].valid) {
      msg = cidr_msg(b.cidr);
      return CYC_ERR_PANIC_CIDR;
    }
    if (!pb.pod_ip[q].valid) {
      msg = "unable to parse IP '" + pb.pod_ip_str[q] + "'";
      return CYC_ERR_PANIC_IP;
    }
    for (uint32_t e = 0; e < b.excnt; e++) {
      uint32_t x = pb.ipb_ex[b.exoff + e];
      if (!pb.cidrs[x].valid) {
        msg = cidr_msg(x);
        return CYC_ERR_PANIC_CIDR;
      }
    }
    return 0;
  };
  // direction 0 (ingress): target d, peer s; direction 1 (egress): target s, peer d
  for (int dir = 0; dir < 2; dir++) {
    uint32_t tp = dir == 0 ? d : s, peer = dir == 0 ? s : d;
    uint32_t ns = pb.pod_ns[tp], ls = pb.pod_ls[tp];
    uint32_t lo = pb.tns_lo[dir][ns], hi = pb.tns_hi[dir][ns];
    for (uint32_t t = lo; t < hi; t++)
      if (sel(pb.tgt[dir][t].sel, ls) == 2) return fail(c, CYC_ERR_PANIC_SELECTOR, "invalid operator");
    // copy of the device outcome rows for the peer pod's word
    for (uint32_t t = lo; t < hi; t++) {
      if (sel(pb.tgt[dir][t].sel, ls) != 1) continue;
      const DTarget& tg = pb.tgt[dir][t];
      for (uint32_t j = tg.poff; j < tg.poff + tg.pcnt; j++) {
        const DPeer& pr = pb.peers[j];
        if (pr.kind == 0) break;
        int32_t de = pb.slot_desc[size_t(d) * pb.K + k];
        std::vector<uint8_t> ok(1);
        HIPCHK(hipMemcpy(ok.data(), prep.portok.as<uint8_t>() + size_t(pr.port) * std::max<size_t>(pb.descs.size(), 1) + de, 1,
                         hipMemcpyDeviceToHost));
        if (pr.kind == 1) {
          if (ok[0]) break;
          continue;
        }
        uint64_t pm, er;
        const size_t row = pr.kind == 3 && j < rp.prow_host.size() ? rp.prow_host[j] : j;  // IP peers share their IPBlock's row
        HIPCHK(hipMemcpy(&pm, prep.PM.as<uint64_t>() + row * pb.W + peer / 64, 8, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(&er, prep.ER.as<uint64_t>() + row * pb.W + peer / 64, 8, hipMemcpyDeviceToHost));
        if ((er >> (peer % 64)) & 1) {
          if (pr.kind == 2) return fail(c, CYC_ERR_PANIC_SELECTOR, "invalid operator");
          std::string msg;
          int code = ip_err(pr, peer, msg);
          return fail(c, code ? code : CYC_ERR_PANIC_CIDR, msg);
        }
        if (((pm >> (peer % 64)) & 1) && ok[0]) break;
      }
    }
  }
  return fail(c, CYC_ERR_PANIC_CIDR, "panic (unresolved message)");
}

static void destroy_events(cyc_ctx* c) {
  for (auto& e : c->run.ev)
    if (e) {
      (void)hipEventDestroy(e);
      e = nullptr;
    }
  for (auto& e : c->run.ev_p)
    if (e) {
      (void)hipEventDestroy(e);
      e = nullptr;
    }
}
