// route.hpp — a run's route: every path decision of one (prepare, option set, row range, partition),
// resolved once from plain facts.  Host C++17 only (no HIP): the engine's headers include it for the
// thresholds, and tests/native/route_check.cpp builds it alone.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>

namespace cyc {

// Most 64-pod words hold 1-2 identity runs (pods of a deployment are contiguous); IDO builds are
// used only when no word holds more than IDO_MAX_RUNS runs (host-checked, plan_peers).
constexpr uint32_t IDO_MAX_RUNS = 4;
constexpr uint32_t IDO_LDS_BYTES = 48 * 1024;       // staged identity sets per class-row block
constexpr uint64_t IDO_B_MAX_BYTES = 1ull << 30;    // both directions' identity-set records (DirDev::B)
constexpr uint32_t PL_NB = 4;                       // wave-per-chunk PM class rows: most descriptors / slots
constexpr uint32_t PL_WAVE_MAX_WORDS = 64 * 64;     // ... and most words (<= 64 chunks)
constexpr uint32_t PORT_BITS_MAX_DESCS = 32;        // descriptor bit rows of the port table: one u32 per matcher
constexpr uint32_t MEMBER_WAVE_MAX_IDENTS = 4096;   // member_wave auto: at most this many active identities
constexpr double MEMBER_WAVE_MIN_TARGETS = 4.0;     // ... each walking at least this many targets on average
constexpr uint64_t POD_SPARSE_MIN_WORDS = 2ull << 20;   // pod_sparse auto: pod-peer words (pod peers x W)
constexpr uint64_t SEL_LAZY_MIN_PAIRS = 64ull << 20;    // sel_lazy auto: (selector, label set) pairs
constexpr uint64_t BIG_PLANE_BYTES = 8ull << 30;        // row_phases / emit_interleave auto: bytes per plane
constexpr uint32_t INPLACE_ROWS_PER_IDENT = 16;         // class_inplace auto: identities >= rows / 16
constexpr uint32_t PHASE_MIN_PODS = 128;                // row phases: fewest pods

// Every settable option (cyc_set_option; what each value means: include/cyclonus_hip.h; what -1 = auto
// chooses: resolve_route, and ensure_range for the two that shape the range plan's IP rows).
struct Options {
  int graphs = -1, front_fused = 1, pod_words = -1, pod_rows = -1, ip_range = -1, ip_iv = -1, member_wave = -1;
  int class_rpb = 0;       // 0 = auto (profiles/r04_class_rpb_ab.txt)
  int pl_wave = 1, sel_lazy = -1, class_inplace = -1, emit_interleave = -1, ip_items = -1;
  int pr_group = -1;       // (a set of 0 is stored as -1)
  int step_events = 0;     // off: the two timing events cost ~9 us of idle GPU per step (config #2 0.077 ->
                           // 0.069 ms/step, profiles/r02_step_events_ab.txt)
  // Row phases: a phase's class rows (~200 MB for config #3) are still in the 256 MB MALL when its emit
  // re-reads them; the whole table's (~400 MB) are not, and its emit reads them from HBM between its
  // writes (round 6, profiles/r06_emit_footprint_ab.txt).  -1 auto, 1 = off, 2 = whenever possible.
  int row_phases = -1;
  int plvt_max_mb = 1024;  // largest PLVT built (0: never, the LVT gathers instead)
};

// What a change of an option makes stale, beyond the route and the captured graph (every set re-resolves
// the one and drops the other).
enum class Stale { nothing, range_plan, plvt };

struct OptionRow {
  const char* name;
  int Options::*field;
  int64_t lo, hi;
  Stale stale;
};
constexpr OptionRow OPTION_TABLE[] = {
    {"graphs", &Options::graphs, -1, 2, Stale::nothing},
    {"front_fused", &Options::front_fused, 0, 1, Stale::nothing},
    {"pod_words", &Options::pod_words, -1, 1, Stale::nothing},
    {"pod_rows", &Options::pod_rows, -1, 1, Stale::nothing},
    {"ip_range", &Options::ip_range, -1, 1, Stale::range_plan},  // which IP rows are range-built
    {"ip_iv", &Options::ip_iv, -1, 1, Stale::range_plan},        // ... and which interval-built
    {"member_wave", &Options::member_wave, -1, 1, Stale::nothing},
    {"class_rpb", &Options::class_rpb, 0, 64, Stale::nothing},
    {"pl_wave", &Options::pl_wave, 0, 1, Stale::nothing},
    {"sel_lazy", &Options::sel_lazy, -1, 1, Stale::nothing},
    {"pr_group", &Options::pr_group, -1, 64, Stale::nothing},
    {"class_inplace", &Options::class_inplace, -1, 1, Stale::nothing},
    {"step_events", &Options::step_events, 0, 1, Stale::nothing},
    {"emit_interleave", &Options::emit_interleave, -1, 1, Stale::nothing},
    {"row_phases", &Options::row_phases, -1, 4, Stale::range_plan},  // the emit lists (of -1..4 only -1, 1, 2 are values)
    {"ip_items", &Options::ip_items, -1, 1, Stale::range_plan},      // the fused front's IP-row items
    {"plvt_max_mb", &Options::plvt_max_mb, 0, 1 << 20, Stale::plvt},
};
inline const OptionRow* find_option(const char* name) {
  for (const OptionRow& r : OPTION_TABLE)
    if (std::strcmp(r.name, name) == 0) return &r;
  return nullptr;
}

// The facts the rules read (the options, the prepared problem, the range plan), nothing else.
struct RouteIn {
  Options opt;
  // the prepared problem
  uint32_t P = 0, K = 0, W = 0;
  uint32_t n_desc = 0, n_pm = 0;  // job descriptors, port matchers
  bool may_err = false;           // a panic is possible
  bool blocks = false;            // batched blocks present
  bool dense_sel = false;
  uint32_t n_sel = 0, L = 0;      // selectors the range reaches, label sets
  bool uni_desc = false;
  uint32_t max_runs = 0;          // most identity runs in one 64-pod word
  uint64_t ido_lds_bytes = 0;     // identity-set rows one class-row block stages
  uint64_t ido_b_bytes = 0;       // identity-set records of both directions
  // the range plan
  uint32_t E = 0;                       // egress identities
  uint32_t rp_off[3] = {0, 0, 0};       // the range's pod peers: ingress, then egress
  uint32_t n_act[2] = {0, 0};           // active identities per direction
  double act_targets[2] = {0, 0};       // mean namespace targets per active identity
  int64_t rows[2] = {0, 0};             // rows per plane
  uint32_t win_w0 = 0, win_wa = 0;      // the ingress word window
  bool whole = false;                   // rows [0, P)
  bool src = false;                     // the rows are sources (CYC_ROWS_SOURCE), not target rows
};

struct Route {
  bool ido = false;          // pod peers folded into per-class identity sets (no PM pod rows)
  bool pod_direct = false;   // pod-peer PM rows per pod directly, not through identity outcomes and word runs
  bool pod_sparse = false;   // PM builds' fused front: sparse pod-peer rows in launch C
  bool fused = false;        // the fused front applies (else the two-branch DAG)
  bool lazy_sel = false;     // selectors evaluated where used, no dense SELRES table
  bool pl_wave = false;      // PM-build class rows a wave per 64-word chunk ("pl_wave_active")
  bool port_bits = false;    // descriptor bit rows of the port table
  bool slot_words = false;   // the fused front builds the slot words
  bool member_wave[2] = {false, false};  // membership a wave per identity
  bool one_window = false;   // both directions' peer rows share one word window
  bool inplace = false;      // class rows written into the output planes (when the run is given both)
  bool emit_interleave = false;  // a target-row emit's row list alternates the planes' rows
  uint32_t phase_split = 0;  // row phases: the split row (0: one pass)
  int launch = 1;            // what cyc_get_option("launch") reports: 1 graph replay, 2 the DAG enqueued eagerly, 0 eager
  bool runs_eager = false;   // the run goes through enqueue_pipeline (one stream, phase events)
};

// Pod peers folded into per-class identity sets, expanded by the class rows over each word's
// identity runs (no PM pod rows)?  Needs: no panic possible (the panic path walks PM / ER rows in
// peer order), few runs per word, and identity sets of bounded size.
inline bool ido_possible(const RouteIn& in) {
  return !in.may_err && in.max_runs <= IDO_MAX_RUNS && in.ido_lds_bytes <= IDO_LDS_BYTES && in.ido_b_bytes <= IDO_B_MAX_BYTES;
}

// The only reader of an option int for a path decision.
inline Route resolve_route(const RouteIn& in) {
  Route r;
  const uint64_t Rp = in.rp_off[2] - in.rp_off[0];  // the range's pod peers
  r.ido = in.opt.pod_words != 0 && !in.blocks && ido_possible(in);
  // "pod_rows": direct when identities >= pods / 2
  r.pod_direct = in.opt.pod_rows >= 0 ? in.opt.pod_rows == 1 : uint64_t(in.E) * 2 >= in.P;
  // The fused front (k_front_a..e, one stream): the same block ranges the two-branch DAG launches
  // as ~15 kernels (enq_common, enq_peer_rows, enq_member, enq_class_rows), grouped by dependency
  // level.  Applies to no-panic builds with dense selectors whose pod-peer rows (PM builds) are
  // computed per pod in one level.
  r.fused = in.opt.front_fused && !in.may_err && in.P && in.K && in.W && !(in.n_sel && in.L && !in.dense_sel) &&
            (r.ido || !(Rp && in.E) || r.pod_direct);
  // PM builds' fused front: sparse pod-peer rows (pod_rows_sparse_blk, launch C) once the rows are
  // large (>= 2M pod-peer words: config #3u), else full rows a wave per (pod peer, word) in launch B,
  // which has the parallelism small problems need (config #2: 125k peer words, B + C 33 vs 52 us).
  // pr_group > 0 forces the sparse rows.
  r.pod_sparse = !r.ido && (in.opt.pr_group > 0 || Rp * in.W >= POD_SPARSE_MIN_WORDS);
  // Selectors evaluated where used (sel_at through LVT), not as the dense SELRES table: the fused
  // front of PM builds (its pod-peer rows and membership are the only selector users, and PM builds
  // are the ones whose label sets number ~ the pods).  The DAG path computes SELRES regardless.
  if (in.dense_sel && !in.may_err && in.opt.sel_lazy != 0 && r.fused) {
    // no pod-peer rows at all (IPBlock-only policies, config #4): the membership is the only selector
    // user, one record and one label-table load per target — no table, and no launch A
    // auto: lazy once the dense table would take ~0.1 ms (>= 64M pairs; config #3u: 0.75G pairs,
    // 1.1 ms; config #2 stays dense — its multi-requirement selectors cost more evaluated per use)
    // IDO builds always: their identity sets and membership evaluate fewer pairs than the table
    // holds (config #3: A + B 118 -> 111 us; its N = 8 shard 35 -> 31 us, profiles/r02_sel_lazy_ab.txt)
    r.lazy_sel = (!Rp && in.opt.sel_lazy < 0) || in.opt.sel_lazy == 1 || r.ido || uint64_t(in.n_sel) * in.L >= SEL_LAZY_MIN_PAIRS;
  }
  // Descriptor bit rows of the port table for the egress class rows
  r.port_bits = std::max<uint32_t>(in.n_desc, 1) <= PORT_BITS_MAX_DESCS;
  // PM-build class rows a wave per 64-word chunk (pl_wave_chunks): both directions' accumulators fit
  // (descriptors and slots <= PL_NB) and every peer's port bits are available.
  r.pl_wave = !r.ido && in.opt.pl_wave && in.K <= PL_NB && in.n_desc <= PL_NB && in.n_desc && in.n_pm && r.port_bits &&
              in.W <= PL_WAVE_MAX_WORDS;
  // the slot words (VALID / DESCW / DM per 64 destinations) serve only egress class rows whose
  // destinations do not all share each slot's descriptor (uni_desc: the UNI class rows read udesc)
  r.slot_words = !in.uni_desc || !(r.ido || r.pl_wave) || in.blocks;
  // auto (-1): a wave per identity while identities are few (<= 4096) and each walks several
  // targets (>= 4 on average): config #3 (2000 identities, ~6 targets each) gains, configs #2
  // (10k identities), #4 (38k) and #5 (~0.3 targets each) lose (profiles/r01_member_wave_ab.txt)
  for (int d = 0; d < 2; d++)
    r.member_wave[d] = in.opt.member_wave > 0 || (in.opt.member_wave < 0 && in.n_act[d] <= MEMBER_WAVE_MAX_IDENTS &&
                                              in.act_targets[d] >= MEMBER_WAVE_MIN_TARGETS);
  // the two directions' peer rows share one window (target-row plans): one launch segment for both
  r.one_window = in.win_w0 == 0 && in.win_wa == in.W;
  // In-place class rows: the fused front with both output planes given.
  // Auto (-1): when the rows' identities are >= 1/16 of the rows (PM builds: config #4 emit -8 %,
  // #3u -7 %), and for identity-set (IDO) runs: config #3's class rows are 2 % of its rows,
  // and writing them into the planes saves their 400 MB of separate writes (3.286 -> 3.191 ms/step,
  // profiles/r05_inplace_sweep_ab.txt; over 5 plane placements in one process -2.1 / -0.0 / -0.1 /
  // -2.8 / -2.2 %, never slower: profiles/r05_plane_placement.txt; a source shard at N = 8 -1.2 %,
  // r05_shard_ab.txt; in round 2, before the current launch E, it lost 1 %).
  if (in.opt.class_inplace && r.fused && !in.blocks) {
    const uint64_t rows = uint64_t(std::max<int64_t>((in.rows[0] + in.rows[1]) / 2, 1));
    r.inplace = in.opt.class_inplace == 1 || uint64_t(in.n_act[0] + in.n_act[1]) * INPLACE_ROWS_PER_IDENT >= 2 * rows || r.ido;
  }
  // alternate the planes' rows when each plane is >= 8 GB (config #3 on one GPU: emit 3.42 ->
  // 3.11 ms on two of three boxes, -1 % on the third; 1-4 % slower for planes of <= 5 GB — 2, 4
  // and 8 shards — profiles/r01_emit_interleave_sweep.txt)
  r.emit_interleave = in.opt.emit_interleave >= 0 ? in.opt.emit_interleave != 0
                                              : uint64_t(in.rows[0]) * in.K * in.win_wa * 8 >= BIG_PLANE_BYTES;
  // row phases (Options::row_phases): a whole no-panic table splits at row P/2 — auto once each plane
  // is >= 8 GB; the emit lists then hold the rows before the split first
  const bool whole = in.whole && (!in.src || in.win_wa == in.W);
  const bool big = uint64_t(in.P) * in.K * in.W * 8 >= BIG_PLANE_BYTES;
  r.phase_split = in.opt.row_phases != 1 && whole && !in.may_err && !in.blocks && in.P >= PHASE_MIN_PODS && (in.opt.row_phases == 2 || big)
                      ? in.P / 2
                      : 0u;
  // "graphs" auto: 2 when the fused front applies (its launches on one stream start ~8 us sooner
  // after the previous step's emit than a graph replay: profiles/r01_front_fused_ab.txt), else 1
  r.launch = in.opt.graphs >= 0 ? in.opt.graphs : (r.fused ? 2 : 1);
  // builds that may panic run enqueue_pipeline whatever "graphs" says (run_pipeline)
  r.runs_eager = in.may_err || r.launch == 0;
  return r;
}

}  // namespace cyc
