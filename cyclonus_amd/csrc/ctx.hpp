// ctx.hpp — the context: device buffers, options, error handling.
// Part of engine.hip's single translation unit (device bodies inline across stages, host helpers are
// static): included once, by engine.hip, in stage order.
#pragma once

// ============================================================================ context + C ABI
using namespace cyc;

#define HIPCHK(x)                                                                   \
  do {                                                                              \
    hipError_t e_ = (x);                                                            \
    if (e_ != hipSuccess) throw HipErr{std::string(#x) + ": " + hipGetErrorString(e_)}; \
  } while (0)

namespace {
struct HipErr {
  std::string msg;
};
struct RcclErr {  // an RCCL call failed (CYC_ERR_RCCL)
  std::string msg;
};

// Makes `device` current for the scope of an entry point and restores the caller's current device
// afterwards: a binding calling in from a thread whose current device is another GPU (e.g. PyTorch
// on cuda:1 with a context on device 0) keeps its own current device.
// Events of a run (stream order, completion, phase timing) release to device scope: a default
// (system-scope) event writes back and invalidates the caches when it is recorded, which left a
// ~15 us idle gap after every step's emit (config #3 timeline, r04c) and inflated the phase timings.
// Nothing here hands memory to the host through an event: host reads are hipMemcpy calls.
constexpr unsigned EV_SYNC = hipEventDisableTiming | hipEventReleaseToDevice;
constexpr unsigned EV_TIMING = hipEventReleaseToDevice;

struct DeviceGuard {
  int prev = -1;
  bool set = false;
  explicit DeviceGuard(int device, bool strict = true) {
    hipError_t e = hipGetDevice(&prev);
    if (e == hipSuccess && prev == device) return;
    e = hipSetDevice(device);
    if (e != hipSuccess) {
      if (strict) throw HipErr{std::string("hipSetDevice: ") + hipGetErrorString(e)};
      return;
    }
    set = prev >= 0;
  }
  ~DeviceGuard() {
    if (set) (void)hipSetDevice(prev);
  }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;
};

struct DevBuf {  // owns a hipMalloc: movable, not copyable
  void* p = nullptr;
  size_t bytes = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr, o.bytes = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      if (p) (void)hipFree(p);
      p = o.p, bytes = o.bytes;
      o.p = nullptr, o.bytes = 0;
    }
    return *this;
  }
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
  void alloc(size_t n) {
    if (p) {
      (void)hipFree(p);
      p = nullptr;
    }
    bytes = n;
    if (n) HIPCHK(hipMalloc(&p, n));
  }
  template <class T>
  T* as() const {
    return static_cast<T*>(p);
  }
};

template <class T>
void upload(DevBuf& b, const std::vector<T>& v) {
  b.alloc(std::max<size_t>(v.size() * sizeof(T), 16));
  if (!v.empty()) HIPCHK(hipMemcpy(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
}

struct Identities {  // pod identities for one direction
  std::vector<uint32_t> ns, ls, nsls, list_off;
  std::vector<int32_t> desc;     // ingress: [n][K]
  std::vector<uint8_t> status;   // ingress: [n][K]
  std::vector<uint32_t> of_pod;  // [P]
  uint64_t list_total = 0;
  uint32_t ht_cap = 0;
};

struct DirDev {
  DevBuf id_ns, id_ls, id_desc, id_status, list_off, list, cnt, hash, err, ht_key, ht_rep, class_of, A, AE, tns_lo,
      tns_hi, tgt, pod_id, reps, B, ip_off, ip_cnt, ip_list;
  uint32_t n = 0, ht_cap = 0;
  // hash table buffer = [cap] u64 keys, [cap] u32 reps, 1 u32 representative counter: one
  // 0xFF memset per run empties the table and sets the counter to ~0 (= count - 1 for 0)
  uint32_t* rep_cnt() { return reinterpret_cast<uint32_t*>(static_cast<char*>(ht_key.p) + uint64_t(ht_cap) * 16); }
};
}  // namespace

struct PeerPlan {
  std::vector<uint32_t> pod_peers, ip_peers, word_off, run_e;
  std::vector<uint64_t> run_mask;
  std::vector<DIPTest> ip_tests;
  std::vector<DCidr> ip_ex;
  uint32_t max_runs = 0;  // most identity runs in one 64-pod word
  std::vector<WordRuns> runs;  // [W] when max_runs <= IDO_MAX_RUNS
};
// The context's state, grouped by the one function that writes each group.

// What a prepare makes (build_identities, prepare_device, prepare_blocks_device, and ensure_plvt on the
// first run that needs the per-pod label table).  A prepare starts from Prepared{}.
struct Prepared {
  Identities ids[2];
  // device tables
  DevBuf ls_off, ls_key, ls_val, sel_off, reqs, req_vals, pod_ns, pod_ls, pod_nsls, pod_ip, cidrs, ipbs, ipb_ex, pms,
      pents, peers, descs, slot_desc, slot_status, slot_cfg, slot_idx;
  DevBuf selres, PM, ER, portok, portbits, VALID, DESCW, DM, first_err;
  DevBuf status_sink;  // status plane target of graph runs given no status pointer (see capture_pipeline)
  // peer-row stage: per-word identity runs, pod-peer outcomes in identity space
  DevBuf id_nsls, word_off, run_e, run_mask, runs, ido, idob, ip_words, zeros, lvt, dreqs;
  DevBuf ip_rng;  // per peer: its IP row's word span and chunk masks, then its nonzero-chunk flags (ip_cnz)
  // ip_rng's span records are all ~0: the last enqueued run's emit reset them (EmitArgs::reset), so the
  // next fused front needs no fill before its IP rows (and, without a selector table, no launch A)
  bool ip_rng_clean = false;
  DevBuf udesc;     // per slot the one VALID descriptor every pod has, when all slots are so (uni_desc)
  bool uni_desc = false;
  DevBuf plvt;      // LVT per pod (SelView::PLVT), built by ensure_plvt when it fits "plvt_max_mb"
  uint32_t n_lkeys = 0;     // dense label keys (LVT rows - 1)
  bool plvt_ready = false;
  DevBuf sel_one;   // SelView::one
  std::vector<uint4> sel_one_h;  // its host copy (the identity-set peer records, RangePlan::pb_rec)
  DevBuf req_post, post_pods;  // label postings: per requirement (offset, count) x 2 values; pod lists
  std::vector<uint8_t> req_post_ok;  // the requirement's pods are its postings (EQ, IN of <= 2 values)
  DevBuf ns_words;  // DWordNS per 64-pod word, then per 64-word chunk (sparse pod rows)
  bool dense_sel = false;  // k_selectors_dense (LVT fits)
  // The address index of the IP rows built from address ranges (ip_rows_range_blk): the pods of each
  // family sorted by address (host keys for the binary searches; the pod order on the device)
  std::vector<uint32_t> ip4_key, ipsort_host;
  std::vector<std::array<uint32_t, 4>> ip6_key;
  DevBuf ipsort;
  std::vector<uint8_t> word_aff;  // per 64-pod word: bit f set when family f's pods there are affine (or absent)
  // IP rows as pod intervals (ip_rows_iv_blk): a family's pods hold non-decreasing addresses in pod order
  // ([0] IPv4, [1] IPv6), so a network less its excepts matches that family's pods in a few pod-index intervals
  bool ip_mono[2] = {false, false};
  std::vector<DWordIP> ipw_h;   // host copy of the IP word and chunk records (ip_words)
  PeerPlan plan;                // all pod / IP peers (host); filtered per row range
  DirDev dir[2];
  // batched blocks (cyc_probe_prepare_blocks; pb.blocks non-empty)
  DevBuf blk, blk_off, id_blk[2], id_win[2], first_blk;
  uint32_t blk_wa_max = 0, blk_np_max = 0;
  std::vector<uint64_t> blk_off_h;  // per block: plane slab offset (words), status offset (bytes); then totals
};

// What ensure_range makes for rows [lo, hi) of a partition, and that key.  A re-plan starts from
// RangePlan{}; whatever makes the plan stale calls invalidate() (the buffers stay until the re-plan).
struct RangePlan {
  int64_t lo = 0, hi = 0;
  bool src = false;  // the plan partitions sources (CYC_ROWS_SOURCE), not target rows
  bool valid = false;
  bool is(int64_t l, int64_t h, bool s) const { return valid && lo == l && hi == h && src == s; }
  void invalidate() { valid = false; }
  // plane rows per direction (ingress keyed by destination, egress by source) and the ingress word
  // window (a source shard's sources: its peers' rows and class rows cover only those words);
  // target-row plans: both directions [lo, hi), window [0, W)
  int64_t rl[2] = {0, 0}, rh[2] = {0, 0};
  uint32_t win_w0 = 0, win_wa = 0;
  uint32_t ido_ew0 = 0, ido_ew1 = 0;  // ingress identity sets: egress-identity words of the window's sources
  DevBuf order[2];                // emit row lists: [rows < Route::phase_split][rows >= it]
  uint32_t phase_n1[2] = {0, 0};  // per plane: rows before the split in its emit list
  DevBuf act[2], actrec[2], sel_list;
  DevBuf arow[2];  // per identity: its first pod's row in the run's row range (in-place class rows)
  uint32_t n_act[2] = {0, 0}, n_sel = 0;
  uint32_t n_act_ph1[2] = {0, 0};  // row phases: active identities whose first row is before the split (every
                                   // phase-1 class's representative is one of them)
  double act_targets[2] = {0, 0};  // mean namespace targets per active identity
  // the range's peers, ingress then egress sub-lists: pod peers, IP peers per pod, range-built and
  // interval-built IP rows
  DevBuf pod_peers, ip_peers, ip_tests, ip_ex, peer_ido, peer_row;
  std::vector<uint32_t> prow_host;  // peer_row on the host (the panic describer reads PM / ER rows by it)
  uint32_t Rp = 0, Ri = 0, Rr = 0, Rv = 0;
  uint32_t rp_off[3] = {0, 0, 0}, ri_off[3] = {0, 0, 0}, rr_off[3] = {0, 0, 0}, rv_off[3] = {0, 0, 0};
  DevBuf ipr_tests, ipr_iv, ipv_tests, ipv_iv;
  // identity-set (IDOB) rows: the needed pod peers, one per distinct (namespace matcher, pod selector) of
  // a direction (peer_ido maps every peer), and per row its matcher as three 16-byte records —
  // (namespace matcher kind, namespace / selector, pod selector, 0), then the namespace selector's and
  // the pod selector's one-requirement records (SelView::one; SEL_ALL when there is none): peer_bits_blk
  // loads a row group's records in one vector load instead of pod_peers -> peers -> one chains
  DevBuf pod_peers_u, pb_rec;
  uint32_t rpu_off[3] = {0, 0, 0};
  DevBuf ido_grp_ns, ido_word_ns;  // identity-set namespace skip (peer_bits_blk): per row group, per identity word
  uint32_t ido_goff[2] = {0, 0};   // first group of each direction's sub-list in ido_grp_ns
  DevBuf pp_scan, pp_post;         // sparse pod rows: pod peers scanned per word / built from postings
  uint32_t n_scan = 0, n_post = 0;
  uint32_t scan_off[3] = {0, 0, 0}, post_off[3] = {0, 0, 0};  // ingress peers, then egress
  DevBuf ipi_items, ipi_list;   // IP-row work items of the fused front (DIPItem; ip_rows_items_blk) and their rows
  uint32_t ipi_off[3] = {0, 0, 0};  // items of segment x: [ipi_off[x], ipi_off[x + 1])
  bool ip_items = false;        // the items are built (option "ip_items" on and fast IP rows present)
};

// What a run writes (run_pipeline and what it enqueues), and the HIP handles runs reuse.  A prepare
// resets `last` and keeps the handles.
struct RunState {
  hipStream_t cap_stream = nullptr, cap_stream2 = nullptr, cap_stream3 = nullptr;  // graph capture branches
  hipEvent_t fork_ev = nullptr, join_ev = nullptr, sel_ev = nullptr, ports_ev = nullptr;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};  // step and phase timing (cyc_last_timings)
  hipEvent_t ev_p[2] = {nullptr, nullptr};  // eager runs: around phase 2's class rows
  hipGraphExec_t graph_exec = nullptr;
  hipGraph_t graph = nullptr;  // kept alive with its exec
  hipEvent_t graph_done = nullptr;  // recorded on the caller's stream after each launch of graph_exec
  const void* graph_key[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  // An exec replaced by a re-capture (new output pointers, row range or tuning knob) may still have
  // a launch queued on the caller's stream: cyc_probe_run returns without synchronising.  It is
  // retired with the event recorded after its last launch and destroyed only once that event has
  // completed (reap_graphs).  Destroying it at once freed an exec a queued launch still used — the
  // intermittent crash inside hipGraphLaunch seen in round 1.
  struct Retired {
    hipGraphExec_t exec;
    hipGraph_t graph;
    hipEvent_t done;  // null: never launched
  };
  std::vector<Retired> retired;
  bool capturing = false;  // a hipGraph capture is in progress (captured steps always fill the spans themselves)
  struct Last {  // the last run of the current prepare
    bool ran = false;    // a run has been enqueued
    hipStream_t stream = nullptr;  // ... on this stream
    bool timed = false;  // it recorded the step timing events
    bool timed_graph = false;
    int phase_used = 0;  // its row phases (2, or 0 for a plain run)
    // what its emit launched (cyc_last_emit): kernel name(s) and launch count
    std::string emit_kernel;
    int emit_launches = 0;
    std::vector<int> blk_rc;           // batched blocks: per block status
    std::vector<std::string> blk_msg;  // and its message
  } last;
};

struct cyc_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  bool have_policy = false, have_res = false, prepared = false;
  PolicyIR policy;
  Resources res;
  Problem pb;  // of the last prepare (build_problem)
  Options opt;
  Prepared prep;
  RangePlan range;
  // The path decisions in effect (route.hpp), re-resolved (reroute) whenever a fact they read changes:
  // by a prepare, by ensure_range and by cyc_set_option — a run only reads them.
  Route route = resolve_route(RouteIn{});
  RunState run;
  // cyc_probe_target_effects' last call (cyc_get_option "effects_*"): how it was batched and the scratch it
  // took.  Nothing of a run reads it.
  struct EffectsLast {
    int64_t batches = 0, launches = 0;  // class batches; (batch, word window) row builds
    uint64_t scratch = 0;               // device bytes held at the peak
  } effects;
  // multi-GPU table assembly (comm.hpp): the context's RCCL communicator, a second stream on which
  // gathered chunks are relaid out under the next chunk's all-gather, and the chunks' double buffer
  struct Comm {
    ncclComm_t nccl = nullptr;
    int nranks = 0, rank = -1;
    hipStream_t merge = nullptr;
    hipEvent_t full[2] = {nullptr, nullptr}, free_[2] = {nullptr, nullptr}, done = nullptr;
    DevBuf scratch[2];
  } comm;
};

int describe_panic(cyc_ctx* c, uint32_t s, uint32_t d, uint32_t cfg, uint32_t idx);
static void comm_release(cyc_ctx* c);  // comm.hpp
static bool rows_layout(const cyc_ctx* c, int part, int64_t lo, int64_t hi, int64_t v[5], std::string& why);

static int fail(cyc_ctx* c, int code, const std::string& m) {
  if (c) c->err = m;
  return code;
}

template <class F>
static int guarded(cyc_ctx* c, F&& f) {
  try {
    return f();
  } catch (Panic& p) {
    return fail(c, p.code, p.msg);
  } catch (HipErr& h) {
    return fail(c, CYC_ERR_HIP, h.msg);
  } catch (RcclErr& r) {
    return fail(c, CYC_ERR_RCCL, r.msg);
  } catch (std::bad_alloc&) {
    return fail(c, CYC_ERR_OOM, "host allocation failed");
  } catch (std::exception& e) {
    return fail(c, CYC_ERR_JSON, e.what());
  }
}

static inline uint64_t hmix(uint64_t z) {  // splitmix64 finaliser (host)
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
