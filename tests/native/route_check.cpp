// route_check.cpp — the path rules of cyclonus_amd/csrc/route.hpp, pinned on the host: each case is a
// RouteIn written out by hand and the answer resolve_route must give, on both sides of every threshold.
// Built with g++ and run by tests/test_route.py; exits non-zero on a mismatch.
#include <cstdio>

#include "route.hpp"

using namespace cyc;

static int failures = 0;
#define EXPECT(in, field, want)                                                                          \
  do {                                                                                                   \
    const long long got_ = (long long)(resolve_route(in).field), want_ = (long long)(want);              \
    if (got_ != want_) {                                                                                 \
      std::printf("%s:%d: %s = %lld, expected %lld\n", __FILE__, __LINE__, #field, got_, want_);         \
      failures++;                                                                                        \
    }                                                                                                    \
  } while (0)

// A small no-panic PM build over all of its 1000 pods: 16 words, 2 slots, 2 descriptors, 3 port
// matchers, dense selectors, 40 pod peers, 600 egress identities (>= P / 2: direct pod rows), 5 runs
// in some word (no identity sets).  The fused front applies.
static RouteIn pm_base() {
  RouteIn in;
  in.P = 1000, in.K = 2, in.W = 16;
  in.n_desc = 2, in.n_pm = 3;
  in.dense_sel = true, in.n_sel = 20, in.L = 700;
  in.max_runs = 5, in.ido_lds_bytes = 2 * 10 * 8, in.ido_b_bytes = 1 << 20;
  in.E = 600;
  in.rp_off[0] = 0, in.rp_off[1] = 15, in.rp_off[2] = 40;
  in.n_act[0] = 500, in.n_act[1] = 600;
  in.act_targets[0] = in.act_targets[1] = 2.0;
  in.rows[0] = in.rows[1] = 1000;
  in.win_w0 = 0, in.win_wa = 16;
  in.whole = true;
  return in;
}
// The same with at most 4 runs per word: identity sets (IDO)
static RouteIn ido_base() {
  RouteIn in = pm_base();
  in.max_runs = IDO_MAX_RUNS;
  return in;
}

static void member_wave() {
  RouteIn in = pm_base();
  in.n_act[0] = 4096, in.act_targets[0] = 4.0;
  in.n_act[1] = 4097, in.act_targets[1] = 4.0;
  EXPECT(in, member_wave[0], 1);
  EXPECT(in, member_wave[1], 0);
  in.n_act[1] = 4096, in.act_targets[1] = 3.999;
  EXPECT(in, member_wave[1], 0);
  in.opt.member_wave = 0;
  EXPECT(in, member_wave[0], 0);
  in.opt.member_wave = 1;
  EXPECT(in, member_wave[1], 1);
}

static void pod_direct() {
  RouteIn in = pm_base();
  in.P = 1200, in.E = 600;  // 2 E == P
  EXPECT(in, pod_direct, 1);
  in.P = 1201;  // 2 E == P - 1
  EXPECT(in, pod_direct, 0);
  in.opt.pod_rows = 1;
  EXPECT(in, pod_direct, 1);
  in.P = 1200, in.opt.pod_rows = 0;
  EXPECT(in, pod_direct, 0);
}

static void pod_sparse() {
  RouteIn in = pm_base();
  in.W = 1 << 11, in.win_wa = in.W;
  in.rp_off[2] = 1024;  // Rp W = 2M
  EXPECT(in, pod_sparse, 1);
  in.rp_off[0] = 1;  // 2M - W; then one word short
  EXPECT(in, pod_sparse, 0);
  in.rp_off[0] = 0, in.rp_off[2] = (1 << 21) - 1, in.W = in.win_wa = 1;  // Rp W = 2M - 1
  EXPECT(in, pod_sparse, 0);
  in.rp_off[2] = 1 << 21;
  EXPECT(in, pod_sparse, 1);
  in = pm_base();
  EXPECT(in, pod_sparse, 0);
  in.opt.pr_group = 8;
  EXPECT(in, pod_sparse, 1);
  in = ido_base();  // never with identity sets
  in.opt.pr_group = 8;
  in.W = in.win_wa = 1 << 11, in.rp_off[2] = 4096;
  EXPECT(in, ido, 1);
  EXPECT(in, pod_sparse, 0);
}

static void lazy_sel() {
  RouteIn in = pm_base();
  EXPECT(in, fused, 1);
  EXPECT(in, lazy_sel, 0);  // pod peers, a small table: dense
  in.rp_off[1] = in.rp_off[2] = 0;  // no pod peers, auto
  EXPECT(in, lazy_sel, 1);
  in.opt.sel_lazy = 0;
  EXPECT(in, lazy_sel, 0);
  in = pm_base();
  in.n_sel = 1 << 13, in.L = 1 << 13;  // 64M pairs
  EXPECT(in, lazy_sel, 1);
  in.L = (1 << 13) - 1;
  EXPECT(in, lazy_sel, 0);
  in.n_sel = (1 << 26) - 1, in.L = 1;  // 64M - 1
  EXPECT(in, lazy_sel, 0);
  in.n_sel = 1 << 26;
  EXPECT(in, lazy_sel, 1);
  in.opt.sel_lazy = 0;
  EXPECT(in, lazy_sel, 0);
  in = pm_base();
  in.opt.sel_lazy = 1;
  EXPECT(in, lazy_sel, 1);
  in.may_err = true;  // never when a panic is possible
  EXPECT(in, lazy_sel, 0);
  in.may_err = false, in.opt.front_fused = 0;  // ... or when the front is not fused
  EXPECT(in, lazy_sel, 0);
  in.opt.front_fused = 1, in.dense_sel = false;  // ... or without the dense label table
  EXPECT(in, fused, 0);
  EXPECT(in, lazy_sel, 0);
  in.n_sel = 0;  // (no selectors at all: fused, still not lazy without dense_sel)
  EXPECT(in, fused, 1);
  EXPECT(in, lazy_sel, 0);
  in = ido_base();
  EXPECT(in, lazy_sel, 1);
  in.opt.sel_lazy = 0;
  EXPECT(in, lazy_sel, 0);
}

static void ido() {
  RouteIn in = ido_base();
  EXPECT(in, ido, 1);
  in.max_runs = IDO_MAX_RUNS + 1;
  EXPECT(in, ido, 0);
  in = ido_base();
  in.may_err = true;
  EXPECT(in, ido, 0);
  in = ido_base();
  in.blocks = true;
  EXPECT(in, ido, 0);
  in = ido_base();
  in.opt.pod_words = 0;
  EXPECT(in, ido, 0);
  in.opt.pod_words = 1;
  EXPECT(in, ido, 1);
  in.max_runs = IDO_MAX_RUNS + 1;  // forcing cannot make it possible
  EXPECT(in, ido, 0);
  in = ido_base();
  in.ido_lds_bytes = IDO_LDS_BYTES;
  EXPECT(in, ido, 1);
  in.ido_lds_bytes = IDO_LDS_BYTES + 1;
  EXPECT(in, ido, 0);
  in = ido_base();
  in.ido_b_bytes = 1ull << 30;
  EXPECT(in, ido, 1);
  in.ido_b_bytes = (1ull << 30) + 1;
  EXPECT(in, ido, 0);
}

static void pl_wave() {
  RouteIn in = pm_base();
  in.K = PL_NB, in.n_desc = PL_NB, in.W = in.win_wa = 4096;
  EXPECT(in, pl_wave, 1);
  EXPECT(in, slot_words, 1);  // (per-destination descriptors)
  in.uni_desc = true;
  EXPECT(in, slot_words, 0);
  in.blocks = true;
  EXPECT(in, slot_words, 1);
  in.blocks = false;
  in.K = PL_NB + 1;
  EXPECT(in, pl_wave, 0);
  EXPECT(in, slot_words, 1);
  in.K = PL_NB, in.n_desc = PL_NB + 1;
  EXPECT(in, pl_wave, 0);
  in.n_desc = PL_NB, in.W = 4097;
  EXPECT(in, pl_wave, 0);
  in.W = 4096, in.opt.pl_wave = 0;
  EXPECT(in, pl_wave, 0);
  in.opt.pl_wave = 1, in.n_pm = 0;
  EXPECT(in, pl_wave, 0);
  in.n_pm = 3, in.n_desc = 0;
  EXPECT(in, pl_wave, 0);
  EXPECT(in, port_bits, 1);
  in.n_desc = 32;
  EXPECT(in, port_bits, 1);
  in.n_desc = 33;
  EXPECT(in, port_bits, 0);
  in = ido_base();  // identity-set runs have no PM class rows
  EXPECT(in, pl_wave, 0);
  in.uni_desc = true;
  EXPECT(in, slot_words, 0);
}

static void fused() {
  RouteIn in = pm_base();
  EXPECT(in, fused, 1);
  in.opt.front_fused = 0;
  EXPECT(in, fused, 0);
  in = pm_base();
  in.may_err = true;
  EXPECT(in, fused, 0);
  for (int z = 0; z < 3; z++) {
    in = pm_base();
    (z == 0 ? in.P : z == 1 ? in.K : in.W) = 0;
    EXPECT(in, fused, 0);
  }
  in = pm_base();
  in.dense_sel = false;  // selectors present, no dense table
  EXPECT(in, fused, 0);
  in = pm_base();
  in.E = 499;  // a PM build needing word-run pod rows
  EXPECT(in, pod_direct, 0);
  EXPECT(in, fused, 0);
  in.rp_off[1] = in.rp_off[2] = 0;  // ... but it has no pod peers
  EXPECT(in, fused, 1);
  in = pm_base();
  in.E = 499, in.max_runs = 3;  // ... or it runs identity sets
  EXPECT(in, fused, 1);
  in.opt.pod_words = 0;
  EXPECT(in, fused, 0);
  in.opt.pod_rows = 1;
  EXPECT(in, fused, 1);
}

static void inplace() {
  RouteIn in = pm_base();
  in.rows[0] = in.rows[1] = 8000;
  in.n_act[0] = 500, in.n_act[1] = 500;  // identities x 16 == 2 rows
  EXPECT(in, inplace, 1);
  in.n_act[1] = 499;
  EXPECT(in, inplace, 0);
  in.opt.class_inplace = 1;
  EXPECT(in, inplace, 1);
  in.opt.class_inplace = 0, in.n_act[1] = 8000;
  EXPECT(in, inplace, 0);
  in.opt.class_inplace = -1;
  EXPECT(in, inplace, 1);
  in.blocks = true;
  EXPECT(in, inplace, 0);
  in.blocks = false, in.opt.front_fused = 0;
  EXPECT(in, inplace, 0);
  in = ido_base();  // identity sets: always, however few identities
  in.rows[0] = in.rows[1] = 1 << 20;
  in.n_act[0] = in.n_act[1] = 1;
  EXPECT(in, inplace, 1);
  in.opt.class_inplace = 0;
  EXPECT(in, inplace, 0);
}

static void phases_and_interleave() {
  RouteIn in = ido_base();
  in.P = 1 << 15, in.K = 64, in.W = in.win_wa = 512;  // P K W 8 = 8 GiB
  in.rows[0] = in.rows[1] = in.P;
  EXPECT(in, phase_split, 1 << 14);
  EXPECT(in, emit_interleave, 1);
  in.K = 63;
  EXPECT(in, phase_split, 0);
  EXPECT(in, emit_interleave, 0);
  in.P = (1 << 30) - 1, in.K = 1, in.W = in.win_wa = 1, in.rows[0] = in.rows[1] = in.P;  // 8 GiB - 8
  EXPECT(in, phase_split, 0);
  EXPECT(in, emit_interleave, 0);
  in.opt.emit_interleave = 1;
  EXPECT(in, emit_interleave, 1);
  in.opt.row_phases = 2;
  EXPECT(in, phase_split, ((1u << 30) - 1) / 2);
  in = ido_base();
  in.P = 1 << 15, in.K = 64, in.W = in.win_wa = 512, in.rows[0] = in.rows[1] = in.P;
  in.opt.emit_interleave = 0;
  EXPECT(in, emit_interleave, 0);
  in.opt.row_phases = 1;
  EXPECT(in, phase_split, 0);
  in.opt.row_phases = -1, in.may_err = true;
  EXPECT(in, phase_split, 0);
  in.may_err = false, in.blocks = true;
  EXPECT(in, phase_split, 0);
  in.blocks = false, in.whole = false, in.rows[0] = in.rows[1] = in.P / 2;  // a row range
  EXPECT(in, phase_split, 0);
  EXPECT(in, emit_interleave, 0);  // (its planes are 4 GiB)
  in.opt.row_phases = 2;
  EXPECT(in, phase_split, 0);
  in.whole = true, in.src = true, in.rows[0] = in.rows[1] = in.P;  // every source: the full window
  EXPECT(in, phase_split, 1 << 14);
  in.win_wa = 511;  // (cannot happen with every source; the rule reads the window)
  EXPECT(in, phase_split, 0);
  in = ido_base();
  in.opt.row_phases = 2, in.P = 128, in.rows[0] = in.rows[1] = 128;
  EXPECT(in, phase_split, 64);
  in.P = 127, in.rows[0] = in.rows[1] = 127;
  EXPECT(in, phase_split, 0);
}

static void launch() {
  for (int fused = 0; fused < 2; fused++)
    for (int may_err = 0; may_err < 2 - fused; may_err++)  // (a build that may panic is never fused)
      for (int g = -1; g <= 2; g++) {
        RouteIn in = pm_base();
        in.opt.front_fused = fused, in.may_err = may_err != 0, in.opt.graphs = g;
        const int want = g >= 0 ? g : fused ? 2 : 1;
        EXPECT(in, fused, fused);
        EXPECT(in, launch, want);
        EXPECT(in, runs_eager, may_err || want == 0);
      }
}

static void one_window() {
  RouteIn in = pm_base();
  EXPECT(in, one_window, 1);
  in.win_wa = 15;
  EXPECT(in, one_window, 0);
  in.win_w0 = 1;
  EXPECT(in, one_window, 0);
}

// The named workloads, whole routes
static void expect_route(const char* name, const RouteIn& in, const Route& w) {
  const Route r = resolve_route(in);
  const bool same = r.ido == w.ido && r.pod_direct == w.pod_direct && r.pod_sparse == w.pod_sparse && r.fused == w.fused &&
                    r.lazy_sel == w.lazy_sel && r.pl_wave == w.pl_wave && r.port_bits == w.port_bits &&
                    r.slot_words == w.slot_words && r.member_wave[0] == w.member_wave[0] &&
                    r.member_wave[1] == w.member_wave[1] && r.one_window == w.one_window && r.inplace == w.inplace &&
                    r.emit_interleave == w.emit_interleave && r.phase_split == w.phase_split && r.launch == w.launch &&
                    r.runs_eager == w.runs_eager;
  if (!same) {
    std::printf("%s: route ido %d direct %d sparse %d fused %d lazy %d pl_wave %d bits %d slot_words %d wave %d %d one_window %d "
                "inplace %d interleave %d split %u launch %d eager %d\n",
                name, r.ido, r.pod_direct, r.pod_sparse, r.fused, r.lazy_sel, r.pl_wave, r.port_bits, r.slot_words,
                r.member_wave[0], r.member_wave[1], r.one_window, r.inplace, r.emit_interleave, r.phase_split, r.launch,
                r.runs_eager);
    failures++;
  }
}

static void workloads() {
  {  // config #2: 10k pods of 10k identities, 1000 policies; PM build with a dense selector table
    RouteIn in;
    in.P = 10000, in.K = 6, in.W = in.win_wa = 157, in.n_desc = 6, in.n_pm = 40;
    in.dense_sel = true, in.n_sel = 1500, in.L = 10000, in.max_runs = 64;
    in.ido_lds_bytes = 6 * 157 * 8, in.ido_b_bytes = 2ull * 10000 * 6 * 157 * 8;
    in.E = 10000, in.rp_off[1] = 400, in.rp_off[2] = 800;
    in.n_act[0] = in.n_act[1] = 10000, in.act_targets[0] = in.act_targets[1] = 10.0;
    in.rows[0] = in.rows[1] = 10000, in.whole = true;
    Route w;
    w.pod_direct = w.fused = w.port_bits = w.slot_words = w.one_window = w.inplace = true;
    w.launch = 2;
    expect_route("config2", in, w);
  }
  RouteIn c3;  // config #3: 100k pods in 2000 identities, 8 slots, 10 GB planes; identity sets
  c3.P = 100000, c3.K = 8, c3.W = c3.win_wa = 1563, c3.n_desc = 8, c3.n_pm = 60;
  c3.dense_sel = true, c3.n_sel = 7460, c3.L = 2994, c3.uni_desc = true, c3.max_runs = 2;
  c3.ido_lds_bytes = 8 * 32 * 8, c3.ido_b_bytes = 2ull * 2000 * 8 * 32 * 8;
  c3.E = 2000, c3.rp_off[1] = 8500, c3.rp_off[2] = 17000;
  c3.n_act[0] = c3.n_act[1] = 2000, c3.act_targets[0] = c3.act_targets[1] = 6.0;
  c3.rows[0] = c3.rows[1] = 100000, c3.whole = true;
  {
    Route w;
    w.ido = w.fused = w.lazy_sel = w.port_bits = w.one_window = w.inplace = w.emit_interleave = true;
    w.member_wave[0] = w.member_wave[1] = true;
    w.phase_split = 50000;
    w.launch = 2;
    expect_route("config3", c3, w);
  }
  {  // its rank 0 of 8 as a source partition: sources [0, 12544), every destination's ingress rows over 196 words
    RouteIn in = c3;
    in.src = true, in.whole = false, in.win_w0 = 0, in.win_wa = 196;
    in.rows[0] = 100000, in.rows[1] = 12544;
    in.n_act[1] = 250, in.rp_off[1] = 8500, in.rp_off[2] = 10600;
    Route w;
    w.ido = w.fused = w.lazy_sel = w.port_bits = w.inplace = true;
    w.member_wave[0] = w.member_wave[1] = true;
    w.launch = 2;
    expect_route("config3 source shard 0 of 8", in, w);
  }
  {  // config #4: 50k pods, 5000 IPBlock-only policies, 4 ports
    RouteIn in;
    in.P = 50000, in.K = 4, in.W = in.win_wa = 782, in.n_desc = 4, in.n_pm = 20;
    in.dense_sel = true, in.n_sel = 5000, in.L = 40000, in.uni_desc = true, in.max_runs = 64;
    in.ido_lds_bytes = 4 * 594 * 8, in.ido_b_bytes = 2ull * 38000 * 4 * 594 * 8;
    in.E = 38000;
    in.n_act[0] = in.n_act[1] = 38000, in.act_targets[0] = in.act_targets[1] = 10.0;
    in.rows[0] = in.rows[1] = 50000, in.whole = true;
    Route w;
    w.pod_direct = w.fused = w.lazy_sel = w.pl_wave = w.port_bits = w.one_window = w.inplace = true;
    w.launch = 2;
    expect_route("config4", in, w);
  }
  {  // config #3u: config #3's policies over pods of unique labels (~an identity per pod)
    RouteIn in = c3;
    in.uni_desc = false, in.max_runs = 64, in.L = 100000;
    in.ido_lds_bytes = 8 * 1563 * 8, in.ido_b_bytes = 2ull * 100000 * 8 * 1563 * 8;
    in.E = 100000, in.n_act[0] = in.n_act[1] = 100000;
    Route w;
    w.pod_direct = w.pod_sparse = w.fused = w.lazy_sel = w.port_bits = w.slot_words = w.one_window = w.inplace = true;
    w.phase_split = 50000, w.emit_interleave = true;  // (its planes are config #3's)
    w.launch = 2;
    expect_route("config3u", in, w);
  }
}

int main() {
  member_wave();
  pod_direct();
  pod_sparse();
  lazy_sel();
  ido();
  pl_wave();
  fused();
  inplace();
  phases_and_interleave();
  launch();
  one_window();
  workloads();
  if (failures) std::printf("%d mismatches\n", failures);
  else std::printf("route rules: ok\n");
  return failures ? 1 : 0;
}
