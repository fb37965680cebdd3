// engine.hip — CDNA4 (gfx950) verdict engine for cyclonus's simulated-connectivity path.
//
// What the reference does per cell (pkg/connectivity/probe/jobrunner.go:68-94 ->
// pkg/matcher/policy.go:131-174): for the ingress direction, walk EVERY ingress target, keep the
// ones whose namespace equals the destination's and whose pod selector matches its labels
// (TargetsApplyingToPod :68-82); the cell is allowed iff no target matched, or some matched
// target's ordered peer list (target.go:29-36) allows the source on the job's port; same for
// egress with source and destination swapped.
//
// What this engine does instead (exact rewriting, no per-cell walk):
//   k_selectors     every (selector, label set) pair once            -> SELRES u8 [S][L]
//   k_peer_rows     every pod/IP peer over all pods as packed bits    -> PM / ER [R][W] u64
//                   (ER = the peer would panic for that pod: bad CIDR/IP/operator)
//   k_portok        every (port matcher, job descriptor)              -> PORTOK u8 [M][D]
//   k_slot_words    per (slot, 64-pod word): valid bits, desc masks   -> VALID, DESCW, DM
//   k_member        per pod IDENTITY (ns, labels[, job descriptors]): matching targets,
//                   a 64-bit hash, and a device hash table that elects one representative
//                   identity per distinct target set                  -> classes
//   k_class_rows    per class representative, slot, word: OR over its targets of the ordered
//                   peer walk done 64 pods at a time with bit ops     -> A_in / A_eg rows
//   k_emit          per target pod: copy its class rows into the output planes (HBM-bound;
//                   the roofline kernel)
//   k_first_error / k_error_detail   only when the inputs can panic: first panicking job in
//                   the reference's job order and the panic message.
#include <dlfcn.h>
#include <execinfo.h>
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <csignal>
#include <cstdlib>
#include <unistd.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <numeric>
#include <string>
#include <unordered_map>
#include <vector>

#include "cyclonus_hip.h"
#include "host.hpp"

// Device code, by stage (namespace cyc)
#include "dev_select.hpp"
#include "dev_peer_rows.hpp"
#include "dev_slots.hpp"
#include "dev_member.hpp"
#include "dev_class_rows.hpp"
#include "dev_front.hpp"
#include "dev_emit.hpp"
#include "dev_query.hpp"
#include "dev_gather.hpp"
#include "dev_table.hpp"
#include "dev_effects.hpp"

// Host side: context, planner, enqueueing; the C ABI below
#include "ctx.hpp"
#include "plan.hpp"
#include "enqueue.hpp"

extern "C" {

const char* cyc_version(void) { return "cyclonus_hip 0.2 (gfx950, ABI 2)"; }
int cyc_abi_version(void) { return CYC_ABI_VERSION; }

// Diagnostic (env CYC_SEGV_TRACE=1): on SIGSEGV print the native frames as module + offset
// (resolve offline with addr2line -e <module> <offset>), then die with the default action.
static void segv_trace(int sig) {
  void* bt[64];
  const int n = backtrace(bt, 64);
  char line[512];
  for (int i = 0; i < n; i++) {
    Dl_info di{};
    int len;
    if (dladdr(bt[i], &di) && di.dli_fname)
      len = snprintf(line, sizeof line, "cyc-segv #%d %s +0x%lx %s\n", i, di.dli_fname,
                     (unsigned long)((char*)bt[i] - (char*)di.dli_fbase), di.dli_sname ? di.dli_sname : "");
    else
      len = snprintf(line, sizeof line, "cyc-segv #%d %p\n", i, bt[i]);
    if (len > 0) (void)!write(2, line, size_t(len));
  }
  signal(sig, SIG_DFL);
  raise(sig);
}

int cyc_ctx_create(int device_id, cyc_ctx** out) {
  if (!out) return CYC_ERR_ARG;
  static const bool trace = [] {
    const char* e = getenv("CYC_SEGV_TRACE");
    if (e && *e == '1') signal(SIGSEGV, segv_trace);
    return true;
  }();
  (void)trace;
  // Policy compilation / IR export work on a host without a GPU: when the device is not there, the
  // context is created without HIP state and the first call that needs it (cyc_probe_prepare) fails.
  // When it is, the context's stream and events are made here — the first HIP stream of a process
  // costs ~100 ms (queue creation), paid once per context instead of inside the first prepare.
  auto* c = new cyc_ctx();
  c->device = device_id;
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) == hipSuccess && device_id >= 0 && device_id < n_dev) {
    DeviceGuard dg(device_id, false);
    int cur = -1;
    bool ok = hipGetDevice(&cur) == hipSuccess && cur == device_id;
    ok = ok && hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) == hipSuccess;
    for (auto& e : c->run.ev) ok = ok && hipEventCreateWithFlags(&e, EV_TIMING) == hipSuccess;
    for (auto& e : c->run.ev_p) ok = ok && hipEventCreateWithFlags(&e, EV_TIMING) == hipSuccess;
    if (!ok) {  // (left to the first prepare, which reports the error)
      for (auto& e : c->run.ev)
        if (e) (void)hipEventDestroy(e), e = nullptr;
      for (auto& e : c->run.ev_p)
        if (e) (void)hipEventDestroy(e), e = nullptr;
      if (c->stream) (void)hipStreamDestroy(c->stream), c->stream = nullptr;
    }
  } else {
    (void)hipGetLastError();  // (no device: nothing to initialise)
  }
  *out = c;
  return (int)CYC_OK;
}

void cyc_ctx_destroy(cyc_ctx* c) {
  if (!c) return;
  if (c->stream) {
    DeviceGuard dg(c->device, false);
    drop_graph(c);
    reap_graphs(c, true);  // waits for each retired exec's last launch only
    destroy_events(c);
    if (c->run.cap_stream) (void)hipStreamDestroy(c->run.cap_stream);
    if (c->run.cap_stream2) (void)hipStreamDestroy(c->run.cap_stream2);
    if (c->run.cap_stream3) (void)hipStreamDestroy(c->run.cap_stream3);
    if (c->run.sel_ev) (void)hipEventDestroy(c->run.sel_ev);
    if (c->run.ports_ev) (void)hipEventDestroy(c->run.ports_ev);
    if (c->run.fork_ev) (void)hipEventDestroy(c->run.fork_ev);
    if (c->run.join_ev) (void)hipEventDestroy(c->run.join_ev);
    comm_release(c);
    (void)hipStreamDestroy(c->stream);
  }
  delete c;
}

const char* cyc_last_error(const cyc_ctx* c) { return c ? c->err.c_str() : "null context"; }

int cyc_policy_build_json(cyc_ctx* c, int simplify, const char* js, size_t len) {
  if (!c || !js) return CYC_ERR_ARG;
  return guarded(c, [&] {
    json::Node n = json::parse(js, len);
    c->policy = build_network_policies(n, simplify != 0);
    c->have_policy = true;
    c->prepared = false;
    return (int)CYC_OK;
  });
}

int cyc_policy_load_ir_json(cyc_ctx* c, const char* js, size_t len) {
  if (!c || !js) return CYC_ERR_ARG;
  return guarded(c, [&] {
    c->policy = load_policy_ir(json::parse(js, len));
    c->have_policy = true;
    c->prepared = false;
    return (int)CYC_OK;
  });
}

// The JSON dumps: bytes needed (+1), the text copied when buf holds it all; -(cyc_status) on failure
// (nothing loaded, or the dump itself failed, e.g. out of memory) with cyc_last_error set.
static int64_t json_out(cyc_ctx* c, bool have, const char* what, const std::function<std::string()>& dump, char* buf,
                        size_t cap) {
  if (!c) return -int64_t(CYC_ERR_ARG);
  if (!have) return -int64_t(fail(c, CYC_ERR_ARG, std::string("no ") + what + " loaded"));
  int64_t need = 0;
  const int rc = guarded(c, [&] {
    const std::string s = dump();
    if (buf && cap > s.size()) {
      memcpy(buf, s.data(), s.size());
      buf[s.size()] = 0;
    }
    need = int64_t(s.size()) + 1;
    return (int)CYC_OK;
  });
  return rc == CYC_OK ? need : -int64_t(rc);
}

int64_t cyc_policy_ir_json(cyc_ctx* c, char* buf, size_t cap) {
  return json_out(c, c && c->have_policy, "policy", [&] { return dump_policy_ir(c->policy); }, buf, cap);
}

int cyc_resources_load_json(cyc_ctx* c, const char* js, size_t len) {
  if (!c || !js) return CYC_ERR_ARG;
  return guarded(c, [&] {
    c->res = load_resources(json::parse(js, len));
    c->have_res = true;
    c->prepared = false;
    return (int)CYC_OK;
  });
}

int64_t cyc_resources_json(cyc_ctx* c, char* buf, size_t cap) {
  return json_out(c, c && c->have_res, "resources", [&] { return dump_resources(c->res); }, buf, cap);
}

int cyc_resources_load(cyc_ctx* c, const cyc_resource_tables* t) {
  if (!c || !t) return CYC_ERR_ARG;
  return guarded(c, [&] {
    c->res = load_resources_tables(*t);
    c->have_res = true;
    c->prepared = false;
    return (int)CYC_OK;
  });
}

int cyc_policy_load(cyc_ctx* c, const cyc_policy_tables* t) {
  if (!c || !t) return CYC_ERR_ARG;
  return guarded(c, [&] {
    c->policy = load_policy_tables(*t);
    c->have_policy = true;
    c->prepared = false;
    return (int)CYC_OK;
  });
}

// `probes` decodes the probe configs (JSON or flat) inside the guarded call
static int probe_prepare(cyc_ctx* c, const std::function<std::vector<ProbeConfig>()>& probes_of, cyc_probe_shape* shape,
                         const std::vector<ProbeBlock>* blocks) {
  if (!c) return CYC_ERR_ARG;
  if (!c->have_policy || !c->have_res) return fail(c, CYC_ERR_ARG, "load a policy and resources first");
  return guarded(c, [&] {
    PhaseClock clk("prepare");
    DeviceGuard dg(c->device);
    clk.lap("device");
    if (!c->stream) {
      HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
      for (auto& e : c->run.ev) HIPCHK(hipEventCreateWithFlags(&e, EV_TIMING));
      for (auto& e : c->run.ev_p) HIPCHK(hipEventCreateWithFlags(&e, EV_TIMING));
    }
    clk.lap("stream");
    const std::vector<ProbeConfig> probes = probes_of();
    c->prepared = false;
    clk.lap("probe configs");
    c->pb = build_problem(c->policy, c->res, probes, blocks);
    clk.lap("build_problem");
    drop_graph(c);
    // nothing of the previous prepare, its range plan or its runs survives (the old buffers are freed
    // before the new ones are allocated); the streams, events and retired execs do
    c->prep = Prepared{};
    c->range = RangePlan{};
    c->run.last = RunState::Last{};
    c->effects = cyc_ctx::EffectsLast{};
    build_identities(c->pb, c->prep);
    clk.lap("identities");
    prepare_device(c);
    clk.lap("device tables");
    c->prepared = true;
    if (shape) {
      shape->pods = c->pb.P;
      shape->slots = c->pb.K;
      shape->words = c->pb.W;
      shape->configs = c->pb.n_cfg;
      shape->targets_in = int64_t(c->pb.tgt[0].size());
      shape->targets_eg = int64_t(c->pb.tgt[1].size());
      shape->peers = int64_t(c->pb.peers.size());
      shape->classes_in = c->prep.dir[0].n;
      shape->classes_eg = c->prep.dir[1].n;
      shape->may_panic = c->pb.may_err ? 1 : 0;
      shape->selectors = c->pb.S;
      shape->label_sets = c->pb.L;
      shape->pod_peers = int64_t(c->prep.plan.pod_peers.size());
      shape->ip_peers = int64_t(c->prep.plan.ip_peers.size());
      shape->descriptors = int64_t(c->pb.descs.size());
      shape->max_word_runs = c->prep.plan.max_runs;
    }
    return (int)CYC_OK;
  });
}

int cyc_probe_prepare(cyc_ctx* c, const char* js, size_t len, cyc_probe_shape* shape) {
  if (!c || !js) return CYC_ERR_ARG;
  return probe_prepare(c, [&] { return load_probes(json::parse(js, len)); }, shape, nullptr);
}

int cyc_probe_prepare_configs(cyc_ctx* c, const cyc_probe_config* cfgs, int64_t n, cyc_probe_shape* shape) {
  if (!c || (n && !cfgs) || n < 0) return CYC_ERR_ARG;
  return probe_prepare(c, [&] { return load_probe_configs(cfgs, n); }, shape, nullptr);
}

int cyc_probe_prepare_blocks(cyc_ctx* c, const char* js, size_t len, const int64_t* block_end, const int32_t* block_config,
                             int64_t n_blocks, cyc_probe_shape* shape) {
  if (!c || !js || n_blocks < 1 || !block_end || !block_config) return CYC_ERR_ARG;
  std::vector<ProbeBlock> bl(static_cast<size_t>(n_blocks));
  int64_t at = 0;
  for (int64_t b = 0; b < n_blocks; b++) {
    if (block_end[b] < at || block_end[b] > int64_t(UINT32_MAX) || block_config[b] < 0)
      return fail(c, CYC_ERR_ARG, "blocks must be consecutive pod ranges with a probe config each");
    bl[size_t(b)] = ProbeBlock{uint32_t(at), uint32_t(block_end[b]), uint32_t(block_config[b])};
    at = block_end[b];
  }
  if (!js) return CYC_ERR_ARG;
  return probe_prepare(c, [&] { return load_probes(json::parse(js, len)); }, shape, &bl);
}

int cyc_blocks_layout(cyc_ctx* c, int64_t* out, int64_t n) {
  if (!c || !out) return CYC_ERR_ARG;
  if (!c->prepared || c->pb.blocks.empty()) return fail(c, CYC_ERR_ARG, "cyc_probe_prepare_blocks first");
  const size_t nb = c->pb.blocks.size();
  if (n < int64_t(nb + 1) * 2) return fail(c, CYC_ERR_ARG, "layout buffer needs 2 * (blocks + 1) entries");
  for (size_t i = 0; i < 2 * (nb + 1); i++) out[i] = int64_t(c->prep.blk_off_h[i]);
  return (int)CYC_OK;
}

int cyc_probe_run_blocks(cyc_ctx* c, void* stream, uint64_t* d_in, uint64_t* d_eg, uint8_t* d_status, int32_t* block_status) {
  if (!c) return CYC_ERR_ARG;
  if (!c->prepared || c->pb.blocks.empty()) return fail(c, CYC_ERR_ARG, "cyc_probe_prepare_blocks first");
  const uint64_t words = c->prep.blk_off_h[2 * c->pb.blocks.size()];
  if ((words && (!d_in || !d_eg)) || !d_status) return fail(c, CYC_ERR_ARG, "null output slab");
  return guarded(c, [&]() -> int {
    DeviceGuard dg(c->device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int rc = run_pipeline(c, st, d_in, d_eg, d_status, 0, c->pb.P, false, false);
    if (rc == CYC_OK && block_status)
      for (size_t b = 0; b < c->run.last.blk_rc.size(); b++) block_status[b] = c->run.last.blk_rc[b];
    return rc;
  });
}

const char* cyc_block_error(const cyc_ctx* c, int64_t b) {
  if (!c || b < 0 || size_t(b) >= c->run.last.blk_msg.size()) return "";
  return c->run.last.blk_msg[size_t(b)].c_str();
}

// The plane pointer contract (include/cyclonus_hip.h): 64-bit words, so 8-byte aligned.  The message
// naming the argument that is not, or null.  Checked on the host before anything is enqueued.
static const char* misaligned_plane(const uint64_t* d_in, const uint64_t* d_eg) {
  if (reinterpret_cast<uintptr_t>(d_in) % 8) return "d_ingress is not 8-byte aligned";
  if (reinterpret_cast<uintptr_t>(d_eg) % 8) return "d_egress is not 8-byte aligned";
  return nullptr;
}

int cyc_probe_run_rows(cyc_ctx* c, void* stream, uint64_t* d_in, uint64_t* d_eg, uint8_t* d_status, int part, int64_t lo,
                       int64_t hi) {
  if (!c) return CYC_ERR_ARG;
  if (!c->prepared) return fail(c, CYC_ERR_ARG, "cyc_probe_prepare first");
  if ((!d_in || !d_eg) && hi > lo) return fail(c, CYC_ERR_ARG, "null output plane");
  if (const char* why = misaligned_plane(d_in, d_eg)) return fail(c, CYC_ERR_ARG, why);
  if (part != CYC_ROWS_TARGET && part != CYC_ROWS_SOURCE) return fail(c, CYC_ERR_ARG, "unknown partition");
  if (!c->pb.blocks.empty()) return fail(c, CYC_ERR_ARG, "context prepared for blocks: use cyc_probe_run_blocks");
  return guarded(c, [&] {
    DeviceGuard dg(c->device);
    hipStream_t st = static_cast<hipStream_t>(stream);  // NULL = the HIP default (null) stream
    return run_pipeline(c, st, d_in, d_eg, d_status, lo, hi, true, part == CYC_ROWS_SOURCE);
  });
}

int cyc_probe_run(cyc_ctx* c, void* stream, uint64_t* d_in, uint64_t* d_eg, uint8_t* d_status, int64_t lo, int64_t hi) {
  return cyc_probe_run_rows(c, stream, d_in, d_eg, d_status, CYC_ROWS_TARGET, lo, hi);
}

int cyc_probe_run_host_rows(cyc_ctx* c, uint64_t* h_in, uint64_t* h_eg, uint8_t* h_status, int part, int64_t lo, int64_t hi) {
  if (!c) return CYC_ERR_ARG;
  if (!c->prepared) return fail(c, CYC_ERR_ARG, "cyc_probe_prepare first");
  return guarded(c, [&]() -> int {
    DeviceGuard dg(c->device);
    int64_t v[5];
    std::string why;
    if (!rows_layout(c, part, lo, hi, v, why)) return fail(c, CYC_ERR_ARG, why);
    const uint64_t words_in = uint64_t(v[0]) * c->pb.K * v[1], words_eg = uint64_t(v[2]) * c->pb.K * v[3];
    DevBuf din, deg, dst;
    din.alloc(std::max<uint64_t>(words_in * 8, 16));
    deg.alloc(std::max<uint64_t>(words_eg * 8, 16));
    dst.alloc(std::max<uint64_t>(uint64_t(c->pb.P) * c->pb.K, 16));
    int rc = run_pipeline(c, c->stream, din.as<uint64_t>(), deg.as<uint64_t>(), dst.as<uint8_t>(), lo, hi, true,
                          part == CYC_ROWS_SOURCE);
    HIPCHK(hipStreamSynchronize(c->stream));
    if (rc != CYC_OK) return rc;
    if (h_in && words_in) HIPCHK(hipMemcpy(h_in, din.p, words_in * 8, hipMemcpyDeviceToHost));
    if (h_eg && words_eg) HIPCHK(hipMemcpy(h_eg, deg.p, words_eg * 8, hipMemcpyDeviceToHost));
    if (h_status && uint64_t(c->pb.P) * c->pb.K)
      HIPCHK(hipMemcpy(h_status, dst.p, uint64_t(c->pb.P) * c->pb.K, hipMemcpyDeviceToHost));
    return (int)CYC_OK;
  });
}

int cyc_probe_run_host(cyc_ctx* c, uint64_t* h_in, uint64_t* h_eg, uint8_t* h_status, int64_t lo, int64_t hi) {
  return cyc_probe_run_host_rows(c, h_in, h_eg, h_status, CYC_ROWS_TARGET, lo, hi);
}

// ---------------------------------------------------------------- which target decides: per-target effect counts
// The batch buffers' cap (dev_effects.hpp).  CYC_EFFECTS_SCRATCH_KB lowers or raises it for one process: a
// development aid like CYC_TRACE_PREPARE, which lets a small problem go through several batches and windows.
static uint64_t effects_scratch_cap() {
  const char* e = getenv("CYC_EFFECTS_SCRATCH_KB");
  if (e && *e) {
    const long long kb = atoll(e);
    if (kb > 0) return uint64_t(kb) << 10;
  }
  return EFF_SCRATCH_CAP;
}

extern "C++" {
namespace {
struct EffClass {  // target pods of the rows with one set of applying targets (ingress: and one descriptor per slot)
  uint32_t list, row, pods;
};
struct EffBatch {
  std::vector<uint32_t> tl;   // its targets, ascending
  std::vector<uint32_t> cls;  // its classes
  uint32_t WA = 0;            // words per window
};
std::string bytes_of(const void* p, size_t n) { return std::string(static_cast<const char*>(p), n); }
}  // namespace

// The call's body (cyc_probe_target_effects checked the arguments and zeroed the outputs; rows, T > 0).
static int target_effects(cyc_ctx* c, int d, int64_t row_lo, int64_t row_hi, int64_t k_lo, int64_t k_hi, int64_t* effects,
                          int64_t* applies) {
  const Problem& pb = c->pb;
  const Prepared& pr = c->prep;
  hipStream_t st = c->stream;
  const uint32_t P = pb.P, K = pb.K, W = pb.W, T = uint32_t(pb.tgt[d].size()), nk = uint32_t(k_hi - k_lo);
  const uint32_t D = uint32_t(std::max<size_t>(pb.descs.size(), 1)), M = uint32_t(pb.pms.size());
  const uint64_t cap = effects_scratch_cap();
  uint64_t fixed = 0, peak = 0;  // scratch: tables alive for the whole call; with the batch buffers
  auto held = [&](const DevBuf& b) { fixed += b.bytes; };
  // CYC_TRACE_PREPARE=1: the call's host phases on stderr, and (synchronising after each) its kernels' times
  PhaseClock clk("effects");
  double k_ms[4] = {0, 0, 0, 0};  // allow rows, population counts, sole sweep, whatever else the stream held
  auto kernel_done = [&](int which) {
    if (!clk.on) return;
    const auto t0 = std::chrono::steady_clock::now();
    HIPCHK(hipStreamSynchronize(st));  // (the launches before it were timed by the previous call)
    k_ms[which] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  };

  // ---- the port table (k_portok), the call's own copy
  DevBuf portok;
  portok.alloc(std::max<uint64_t>(uint64_t(M) * D, 16));
  held(portok);
  const PortArgs pa{grid1(uint64_t(M) * D, 256), M, D, pr.pms.as<DPortM>(), pr.pents.as<DPortEntry>(), pr.descs.as<DDesc>(),
                    portok.as<uint8_t>()};
  if (pa.nb) k_portok<<<pa.nb, 256, 0, st>>>(pa);
  HIPCHK(hipGetLastError());

  EffTables x{};
  x.P = P, x.K = K, x.W = W, x.D = D;
  x.pod_ns = pr.pod_ns.as<uint32_t>(), x.pod_ls = pr.pod_ls.as<uint32_t>(), x.pod_nsls = pr.pod_nsls.as<uint32_t>();
  x.pod_ip = pr.pod_ip.as<DIP>();
  x.sel_off = pr.sel_off.as<uint32_t>(), x.req_vals = pr.req_vals.as<uint32_t>(), x.reqs = pr.reqs.as<DReq>();
  x.ls_off = pr.ls_off.as<uint32_t>(), x.ls_key = pr.ls_key.as<uint32_t>(), x.ls_val = pr.ls_val.as<uint32_t>();
  x.peers = pr.peers.as<DPeer>(), x.ipbs = pr.ipbs.as<DIPBlock>(), x.cidrs = pr.cidrs.as<DCidr>();
  x.ipb_ex = pr.ipb_ex.as<uint32_t>();
  x.tgt = pr.dir[d].tgt.as<DTarget>(), x.tns_lo = pr.dir[d].tns_lo.as<uint32_t>(), x.tns_hi = pr.dir[d].tns_hi.as<uint32_t>();
  x.slot_desc = pr.slot_desc.as<int32_t>(), x.slot_status = pr.slot_status.as<uint8_t>();
  x.portok = portok.as<uint8_t>();

  // ---- TargetsApplyingToPod once per distinct (namespace, label set) of the rows' pods
  const uint32_t rows = uint32_t(row_hi - row_lo);
  std::vector<uint32_t> id_ns, id_ls, id_pods, pod_id(rows);
  {
    std::unordered_map<uint64_t, uint32_t> id_of;
    for (uint32_t r = 0; r < rows; r++) {
      const uint32_t q = uint32_t(row_lo) + r;
      auto it = id_of.emplace(uint64_t(pb.pod_ns[q]) << 32 | pb.pod_ls[q], uint32_t(id_ns.size()));
      if (it.second) id_ns.push_back(pb.pod_ns[q]), id_ls.push_back(pb.pod_ls[q]), id_pods.push_back(0);
      pod_id[r] = it.first->second;
      id_pods[pod_id[r]]++;
    }
  }
  const uint32_t n_id = uint32_t(id_ns.size());
  std::vector<uint32_t> cnt(n_id), off(n_id + 1, 0), list;
  {
    DevBuf d_ns, d_ls, d_cnt, d_off, d_list;
    upload(d_ns, id_ns);
    upload(d_ls, id_ls);
    d_cnt.alloc(uint64_t(n_id) * 4);
    EffMemberArgs ma{};
    ma.x = x, ma.n = n_id, ma.id_ns = d_ns.as<uint32_t>(), ma.id_ls = d_ls.as<uint32_t>(), ma.cnt = d_cnt.as<uint32_t>();
    k_eff_member<false><<<grid1(uint64_t(n_id) * 64, 256), 256, 0, st>>>(ma);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(cnt.data(), d_cnt.p, uint64_t(n_id) * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    uint64_t tot = 0;
    for (uint32_t i = 0; i < n_id; i++) {
      off[i] = uint32_t(tot);
      tot += cnt[i];
      if (tot > 0xFFFFFFFFull) throw Panic{CYC_ERR_OOM, "target effects: the rows' applying-target lists exceed 2^32 entries"};
    }
    off[n_id] = uint32_t(tot);
    list.resize(tot);
    if (tot) {
      upload(d_off, off);
      d_list.alloc(tot * 4);
      ma.off = d_off.as<uint32_t>(), ma.list = d_list.as<uint32_t>();
      k_eff_member<true><<<grid1(uint64_t(n_id) * 64, 256), 256, 0, st>>>(ma);
      HIPCHK(hipGetLastError());
      HIPCHK(hipMemcpyAsync(list.data(), d_list.p, tot * 4, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
    }
    peak = fixed + d_ns.bytes + d_ls.bytes + d_cnt.bytes + d_off.bytes + d_list.bytes;
  }
  clk.lap("membership");
  if (applies)
    for (uint32_t i = 0; i < n_id; i++)
      for (uint32_t e = off[i]; e < off[i + 1]; e++) applies[list[e]] += id_pods[i];
  c->effects.scratch = peak;
  if (!nk) return (int)CYC_OK;

  // ---- classes: (applying-target list, ingress: the slots' VALID descriptors) -> pods of the rows
  std::vector<uint32_t> lid_of(n_id), l_off, l_len;  // distinct lists: a representative's span in `list`
  {
    std::unordered_map<std::string, uint32_t> seen;
    for (uint32_t i = 0; i < n_id; i++) {
      auto it = seen.emplace(bytes_of(list.data() + off[i], size_t(cnt[i]) * 4), uint32_t(l_off.size()));
      if (it.second) l_off.push_back(off[i]), l_len.push_back(cnt[i]);
      lid_of[i] = it.first->second;
    }
  }
  std::vector<int32_t> row_desc;  // [distinct rows][nk]: the slot's descriptor when its job is VALID, else -1
  std::vector<EffClass> cls;
  {
    std::unordered_map<std::string, uint32_t> seen_row;
    std::unordered_map<uint64_t, uint32_t> seen_cls;
    std::vector<int32_t> rd(nk);
    for (uint32_t r = 0; r < rows; r++) {
      const uint32_t q = uint32_t(row_lo) + r, lid = lid_of[pod_id[r]];
      if (!l_len[lid]) continue;  // no target applies: no effect to count
      uint32_t rid = 0;
      if (d == 0) {
        for (uint32_t kk = 0; kk < nk; kk++) {
          const size_t at = size_t(q) * K + size_t(k_lo) + kk;
          rd[kk] = pb.slot_status[at] == CYC_JOB_VALID ? pb.slot_desc[at] : -1;
        }
        auto it = seen_row.emplace(bytes_of(rd.data(), size_t(nk) * 4), uint32_t(seen_row.size()));
        if (it.second) row_desc.insert(row_desc.end(), rd.begin(), rd.end());
        rid = it.first->second;
      }
      auto it = seen_cls.emplace(uint64_t(lid) << 32 | rid, uint32_t(cls.size()));
      if (it.second) cls.push_back(EffClass{lid, rid, 0});
      cls[it.first->second].pods++;
    }
  }
  if (cls.empty()) return (int)CYC_OK;
  // classes of one namespace side by side (their targets are one run of the primary-key order)
  std::sort(cls.begin(), cls.end(), [&](const EffClass& a, const EffClass& b) {
    const uint32_t fa = list[l_off[a.list]], fb = list[l_off[b.list]];
    return fa != fb ? fa < fb : a.list != b.list ? a.list < b.list : a.row < b.row;
  });

  clk.lap("classes");
  // ---- egress: the VALID pods of every (slot, descriptor) as bit rows, and their number per slot
  std::vector<int64_t> n_valid(nk, 0);
  DevBuf V;
  if (d == 1) {
    for (uint32_t q = 0; q < P; q++)
      for (uint32_t kk = 0; kk < nk; kk++) n_valid[kk] += pb.slot_status[size_t(q) * K + size_t(k_lo) + kk] == CYC_JOB_VALID;
    V.alloc(std::max<uint64_t>(uint64_t(nk) * D * W * 8, 16));
    held(V);
    EffValidArgs va{x, uint32_t(k_lo), nk, V.as<uint64_t>()};
    k_eff_valid<<<grid1(uint64_t(nk) * W * 64, 256), 256, 0, st>>>(va);
    HIPCHK(hipGetLastError());
  }

  // ---- batches: classes in order while the union of their targets' rows fits the cap; a batch of one class
  // that does not fit whole is built a window of words at a time
  const uint32_t X = d == 0 ? D : nk;  // population counts per target
  const uint64_t per_t = uint64_t(X + nk) * 8, per_tw = uint64_t(D) * 8;  // bytes per target; per target and word
  std::vector<EffBatch> batches;
  {
    std::vector<uint32_t> stamp(T, 0);
    for (uint32_t ci = 0; ci < cls.size(); ci++) {
      const uint32_t* L = list.data() + l_off[cls[ci].list];
      const uint32_t n = l_len[cls[ci].list];
      for (int attempt = 0; attempt < 2; attempt++) {
        if (batches.empty() || attempt) batches.emplace_back();
        EffBatch& b = batches.back();
        const uint32_t id = uint32_t(batches.size());
        uint32_t fresh = 0;
        for (uint32_t e = 0; e < n; e++) fresh += stamp[L[e]] != id;
        const uint64_t U = b.tl.size() + fresh;
        if (!b.cls.empty() && U * (per_t + per_tw * W) > cap) continue;  // (a new batch takes it)
        if (U * (per_t + per_tw) > cap)
          throw Panic{CYC_ERR_OOM, "target effects: " + std::to_string(U) + " targets apply to one pod; their rows of one word exceed the scratch cap"};
        for (uint32_t e = 0; e < n; e++)
          if (stamp[L[e]] != id) stamp[L[e]] = id, b.tl.push_back(L[e]);
        b.cls.push_back(ci);
        break;
      }
    }
    for (EffBatch& b : batches) {
      std::sort(b.tl.begin(), b.tl.end());
      const uint64_t U = b.tl.size();
      b.WA = uint32_t(std::min<uint64_t>(W, (cap - U * per_t) / (U * per_tw)));
    }
  }

  // ---- the batch buffers, sized for the largest batch
  uint64_t max_a = 0, max_u = 0, max_ct = 0, max_c = 0;
  for (const EffBatch& b : batches) {
    max_a = std::max<uint64_t>(max_a, uint64_t(b.tl.size()) * D * b.WA);
    max_u = std::max<uint64_t>(max_u, b.tl.size());
    uint64_t ct = 0;
    for (uint32_t ci : b.cls) ct += l_len[cls[ci].list];
    max_ct = std::max(max_ct, ct);
    max_c = std::max<uint64_t>(max_c, b.cls.size());
  }
  DevBuf d_a, d_pop, d_sole, d_tl, d_coff, d_ct, d_cn, d_cd;
  d_a.alloc(max_a * 8);
  d_pop.alloc(max_u * X * 8);
  d_sole.alloc(max_u * nk * 8);
  d_tl.alloc(max_u * 4);
  d_coff.alloc((max_c + 1) * 4);
  d_ct.alloc(max_ct * 4);
  d_cn.alloc(max_c * 4);
  d_cd.alloc(std::max<uint64_t>(max_c * nk * 4, 16));
  peak = std::max(peak, fixed + d_a.bytes + d_pop.bytes + d_sole.bytes + d_tl.bytes + d_coff.bytes + d_ct.bytes + d_cn.bytes + d_cd.bytes);
  c->effects.scratch = peak;

  // effects[.][1] and [.][3] hold the applicable VALID cells (of all classes; of one-target classes) until
  // the end; allow1 the ALLOWING cells of one-target classes
  std::vector<int64_t> allow1(size_t(T) * nk, 0);
  std::vector<uint32_t> loc(T, 0), coff, ct, cn;
  std::vector<int32_t> cd;
  std::vector<unsigned long long> pop, sole;
  for (const EffBatch& b : batches) {
    const uint32_t U = uint32_t(b.tl.size());
    for (uint32_t u = 0; u < U; u++) loc[b.tl[u]] = u;
    // the classes of two or more targets, for the sole sweep
    coff.assign(1, 0), ct.clear(), cn.clear(), cd.clear();
    for (uint32_t ci : b.cls) {
      const EffClass& k = cls[ci];
      const uint32_t* L = list.data() + l_off[k.list];
      const uint32_t n = l_len[k.list];
      for (uint32_t kk = 0; kk < nk; kk++) {  // the applicable VALID cells (window-independent)
        const int64_t cells = d == 0 ? (row_desc[size_t(k.row) * nk + kk] >= 0 ? int64_t(P) : 0) : n_valid[kk];
        for (uint32_t e = 0; e < n; e++) {
          int64_t* o = effects + (size_t(L[e]) * nk + kk) * 4;
          o[CYC_EFFECT_DENYING] += cells * k.pods;
          if (n == 1) o[CYC_EFFECT_SOLE_DENYING] += cells * k.pods;
        }
      }
      if (n < 2) continue;
      for (uint32_t e = 0; e < n; e++) ct.push_back(loc[L[e]]);
      coff.push_back(uint32_t(ct.size()));
      cn.push_back(k.pods);
      if (d == 0) cd.insert(cd.end(), row_desc.begin() + size_t(k.row) * nk, row_desc.begin() + size_t(k.row + 1) * nk);
    }
    const uint32_t NC = uint32_t(cn.size());
    HIPCHK(hipMemcpyAsync(d_tl.p, b.tl.data(), size_t(U) * 4, hipMemcpyHostToDevice, st));
    if (NC) {
      HIPCHK(hipMemcpyAsync(d_coff.p, coff.data(), coff.size() * 4, hipMemcpyHostToDevice, st));
      HIPCHK(hipMemcpyAsync(d_ct.p, ct.data(), ct.size() * 4, hipMemcpyHostToDevice, st));
      HIPCHK(hipMemcpyAsync(d_cn.p, cn.data(), cn.size() * 4, hipMemcpyHostToDevice, st));
      if (d == 0) HIPCHK(hipMemcpyAsync(d_cd.p, cd.data(), cd.size() * 4, hipMemcpyHostToDevice, st));
    }
    pop.resize(size_t(U) * X);
    sole.resize(size_t(U) * nk);
    for (uint32_t w0 = 0; w0 < W; w0 += b.WA) {
      const uint32_t WA = std::min(b.WA, W - w0);
      EffRowArgs ra{x, U, w0, WA, d_tl.as<uint32_t>(), d_a.as<uint64_t>()};
      kernel_done(3);  // (uploads, k_eff_valid)
      k_eff_rows<<<grid1(uint64_t(U) * WA * 64, 256), 256, 0, st>>>(ra);
      HIPCHK(hipGetLastError());
      kernel_done(0);
      EffPopArgs pa2{D, W, w0, WA, X, d_a.as<uint64_t>(), V.as<uint64_t>(), d_pop.as<unsigned long long>()};
      if (d == 0) k_eff_pop<false><<<unsigned(uint64_t(U) * X), 256, 0, st>>>(pa2);
      else k_eff_pop<true><<<unsigned(uint64_t(U) * X), 256, 0, st>>>(pa2);
      HIPCHK(hipGetLastError());
      kernel_done(1);
      if (NC) {
        HIPCHK(hipMemsetAsync(d_sole.p, 0, size_t(U) * nk * 8, st));
        EffSoleArgs sa{D, W, w0, WA, nk, NC, d_a.as<uint64_t>(), V.as<uint64_t>(), d_coff.as<uint32_t>(), d_ct.as<uint32_t>(),
                       d_cn.as<uint32_t>(), d_cd.as<int32_t>(), d_sole.as<unsigned long long>()};
        const unsigned nb = grid1(uint64_t(NC) * nk * ((WA + 255) / 256), 1);
        if (d == 0) k_eff_sole<false><<<nb, 256, 0, st>>>(sa);
        else k_eff_sole<true><<<nb, 256, 0, st>>>(sa);
        HIPCHK(hipGetLastError());
        kernel_done(2);
        HIPCHK(hipMemcpyAsync(sole.data(), d_sole.p, sole.size() * 8, hipMemcpyDeviceToHost, st));
      }
      HIPCHK(hipMemcpyAsync(pop.data(), d_pop.p, pop.size() * 8, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      c->effects.launches++;
      for (uint32_t ci : b.cls) {
        const EffClass& k = cls[ci];
        const uint32_t* L = list.data() + l_off[k.list];
        const uint32_t n = l_len[k.list];
        for (uint32_t kk = 0; kk < nk; kk++) {
          const int32_t j = d == 0 ? row_desc[size_t(k.row) * nk + kk] : int32_t(kk);
          if (j < 0) continue;
          for (uint32_t e = 0; e < n; e++) {
            const int64_t v = int64_t(pop[size_t(loc[L[e]]) * X + uint32_t(j)]) * k.pods;
            effects[(size_t(L[e]) * nk + kk) * 4 + CYC_EFFECT_ALLOWING] += v;
            if (n == 1) allow1[size_t(L[e]) * nk + kk] += v;
          }
        }
      }
      if (NC)
        for (uint32_t u = 0; u < U; u++)
          for (uint32_t kk = 0; kk < nk; kk++)
            effects[(size_t(b.tl[u]) * nk + kk) * 4 + CYC_EFFECT_SOLE_ALLOWING] += int64_t(sole[size_t(u) * nk + kk]);
    }
    c->effects.batches++;
  }
  clk.lap("batches");
  if (clk.on)
    fprintf(stderr, "[cyc effects] %lld batches, %lld row builds, %zu classes: k_eff_rows %.2f ms, k_eff_pop %.2f ms, k_eff_sole %.2f ms, other %.2f ms\n",
            (long long)c->effects.batches, (long long)c->effects.launches, cls.size(), k_ms[0], k_ms[1], k_ms[2], k_ms[3]);
  for (size_t i = 0; i < size_t(T) * nk; i++) {
    effects[i * 4 + CYC_EFFECT_DENYING] -= effects[i * 4 + CYC_EFFECT_ALLOWING];
    effects[i * 4 + CYC_EFFECT_SOLE_DENYING] -= allow1[i];
  }
  return (int)CYC_OK;
}
}  // extern "C++"

int cyc_probe_target_effects(cyc_ctx* c, int direction, int64_t row_lo, int64_t row_hi, int64_t k_lo, int64_t k_hi, int64_t* effects,
                             int64_t* applies) {
  if (!c) return CYC_ERR_ARG;
  if (!c->prepared) return fail(c, CYC_ERR_ARG, "cyc_probe_prepare first");
  if (!c->pb.blocks.empty()) return fail(c, CYC_ERR_ARG, "context prepared for blocks: target effects need cyc_probe_prepare");
  if (direction != CYC_DIR_INGRESS && direction != CYC_DIR_EGRESS) return fail(c, CYC_ERR_ARG, "unknown direction");
  if (row_lo < 0 || row_hi > int64_t(c->pb.P) || row_lo > row_hi) return fail(c, CYC_ERR_ARG, "row range out of bounds");
  if (k_lo < 0 || k_hi > int64_t(c->pb.K) || k_lo > k_hi) return fail(c, CYC_ERR_ARG, "slot range out of bounds");
  if (!effects) return fail(c, CYC_ERR_ARG, "null effects");
  if (c->pb.may_err)
    return fail(c, CYC_ERR_ARG,
                "the problem can panic (may_panic): take the panic from cyc_probe_run; the reference would die at its first such job");
  const int64_t T = int64_t(c->pb.tgt[direction].size());
  std::fill(effects, effects + T * (k_hi - k_lo) * 4, int64_t(0));
  if (applies) std::fill(applies, applies + T, int64_t(0));
  c->effects = cyc_ctx::EffectsLast{};
  if (!T || row_lo == row_hi) return (int)CYC_OK;
  return guarded(c, [&]() -> int {
    DeviceGuard dg(c->device);
    return target_effects(c, direction, row_lo, row_hi, k_lo, k_hi, effects, applies);
  });
}

// ---------------------------------------------------------------- device-resident tables
struct cyc_table {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  uint32_t P = 0, K = 0, W = 0;
  int64_t row_lo = 0, row_hi = 0;
  int partition = CYC_ROWS_TARGET;  // CYC_ROWS_SOURCE: rows are sources; ingress rows cover words [w0, w0 + wa)
  uint32_t w0 = 0, wa = 0;
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
  v[0] = src ? P : hi - lo;
  v[1] = wa;
  v[2] = hi - lo;
  v[3] = W;
  v[4] = src ? lo / 64 : 0;
  return true;
}

static int table_new(cyc_ctx* c, int part, int64_t lo, int64_t hi, cyc_table** out) {
  int64_t v[5];
  std::string why;
  if (!rows_layout(c, part, lo, hi, v, why)) return fail(c, CYC_ERR_ARG, why);
  auto* t = new cyc_table();
  t->device = c->device;
  t->P = c->pb.P;
  t->K = c->pb.K;
  t->W = c->pb.W;
  t->row_lo = lo;
  t->row_hi = hi;
  t->partition = part;
  t->w0 = uint32_t(v[4]);
  t->wa = uint32_t(v[1]);
  *out = t;
  return (int)CYC_OK;
}

int cyc_table_run_rows(cyc_ctx* c, int part, int64_t lo, int64_t hi, cyc_table** out) {
  if (!c || !out) return CYC_ERR_ARG;
  *out = nullptr;
  if (!c->prepared) return fail(c, CYC_ERR_ARG, "cyc_probe_prepare first");
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
    t->in = t->own_in.as<uint64_t>();
    t->eg = t->own_eg.as<uint64_t>();
    t->status = t->own_st.as<uint8_t>();
    rc = run_pipeline(c, c->stream, t->own_in.as<uint64_t>(), t->own_eg.as<uint64_t>(), t->own_st.as<uint8_t>(), lo, hi,
                      false, part == CYC_ROWS_SOURCE);
    HIPCHK(hipStreamSynchronize(c->stream));
    if (rc != CYC_OK) return rc;
    *out = hold.release();
    return (int)CYC_OK;
  });
}

int cyc_table_run(cyc_ctx* c, int64_t lo, int64_t hi, cyc_table** out) { return cyc_table_run_rows(c, CYC_ROWS_TARGET, lo, hi, out); }

int cyc_table_wrap_rows(cyc_ctx* c, const uint64_t* d_in, const uint64_t* d_eg, const uint8_t* d_status, int part, int64_t lo,
                        int64_t hi, cyc_table** out) {
  if (!c || !out) return CYC_ERR_ARG;
  *out = nullptr;
  if (!c->prepared) return fail(c, CYC_ERR_ARG, "cyc_probe_prepare first");
  if (!d_status || ((!d_in || !d_eg) && hi > lo)) return fail(c, CYC_ERR_ARG, "null plane");
  if (const char* why = misaligned_plane(d_in, d_eg)) return fail(c, CYC_ERR_ARG, why);
  cyc_table* t = nullptr;
  int rc = table_new(c, part, lo, hi, &t);
  if (rc != CYC_OK) return rc;
  t->in = d_in;
  t->eg = d_eg;
  t->status = d_status;
  *out = t;
  return (int)CYC_OK;
}

int cyc_table_wrap(cyc_ctx* c, const uint64_t* d_in, const uint64_t* d_eg, const uint8_t* d_status, int64_t lo, int64_t hi,
                   cyc_table** out) {
  return cyc_table_wrap_rows(c, d_in, d_eg, d_status, CYC_ROWS_TARGET, lo, hi, out);
}

int cyc_rows_layout(cyc_ctx* c, int part, int64_t lo, int64_t hi, int64_t* out, int n) {
  if (!c || !out) return CYC_ERR_ARG;
  if (!c->prepared) return fail(c, CYC_ERR_ARG, "cyc_probe_prepare first");
  int64_t v[5];
  std::string why;
  if (!rows_layout(c, part, lo, hi, v, why)) return fail(c, CYC_ERR_ARG, why);
  for (int i = 0; i < n && i < 5; i++) out[i] = v[i];
  return (int)CYC_OK;
}

const char* cyc_table_error(const cyc_table* t) { return t ? t->err.c_str() : "null table"; }

int cyc_table_shape(const cyc_table* t, int64_t* out, int n) {
  if (!t || !out) return CYC_ERR_ARG;
  const int64_t v[8] = {t->P, t->K, t->W, t->row_lo, t->row_hi, t->partition, t->w0, t->wa};
  for (int i = 0; i < n && i < 8; i++) out[i] = v[i];
  return (int)CYC_OK;
}

int cyc_table_cells(cyc_table* t, int64_t s_lo, int64_t s_hi, int64_t d_lo, int64_t d_hi, int64_t k_lo, int64_t k_hi,
                    uint8_t* ingress, uint8_t* egress, uint8_t* combined) {
  if (!t) return CYC_ERR_ARG;
  auto bad = [&](const char* m) {
    t->err = m;
    return (int)CYC_ERR_ARG;
  };
  if (s_lo < 0 || s_hi > int64_t(t->P) || s_lo > s_hi || d_lo < 0 || d_hi > int64_t(t->P) || d_lo > d_hi || k_lo < 0 ||
      k_hi > int64_t(t->K) || k_lo > k_hi)
    return bad("cell range out of bounds");
  // ingress rows are keyed by destination, egress rows by source (include/cyclonus_hip.h); a
  // source-row table holds both directions of its sources' cells
  const bool src = t->partition == CYC_ROWS_SOURCE;
  const bool need_d = !src && (ingress || combined), need_s = egress || combined || (src && ingress);
  if (s_hi > s_lo && d_hi > d_lo && k_hi > k_lo) {
    if (need_d && (d_lo < t->row_lo || d_hi > t->row_hi)) return bad("ingress cells need destinations inside the table's rows");
    if (need_s && (s_lo < t->row_lo || s_hi > t->row_hi))
      return bad(src ? "cells of a source-row table need sources inside its rows" : "egress cells need sources inside the table's rows");
  }
  const uint64_t n = uint64_t(s_hi - s_lo) * uint64_t(d_hi - d_lo) * uint64_t(k_hi - k_lo);
  if (!n) return (int)CYC_OK;
  try {
    DeviceGuard dg(t->device);
    if (!t->stream) HIPCHK(hipStreamCreateWithFlags(&t->stream, hipStreamNonBlocking));
    DevBuf o[3];
    uint8_t* host[3] = {ingress, egress, combined};
    for (int x = 0; x < 3; x++)
      if (host[x]) o[x].alloc(n);
    CellArgs a{};
    a.K = t->K;
    a.W = t->W;
    a.row_lo = uint32_t(t->row_lo);
    a.row_hi = uint32_t(t->row_hi);
    a.src = src ? 1u : 0u;
    a.w0 = t->w0;
    a.WA = t->wa;
    a.in = t->in;
    a.eg = t->eg;
    a.status = t->status;
    a.s_lo = uint32_t(s_lo);
    a.d_lo = uint32_t(d_lo);
    a.k_lo = uint32_t(k_lo);
    a.nd = uint32_t(d_hi - d_lo);
    a.nk = uint32_t(k_hi - k_lo);
    a.n = n;
    a.o_in = o[0].as<uint8_t>();
    a.o_eg = o[1].as<uint8_t>();
    a.o_comb = o[2].as<uint8_t>();
    k_table_cells<<<grid1(n, 256), 256, 0, t->stream>>>(a);
    HIPCHK(hipGetLastError());
    for (int x = 0; x < 3; x++)
      if (host[x]) HIPCHK(hipMemcpyAsync(host[x], o[x].p, n, hipMemcpyDeviceToHost, t->stream));
    HIPCHK(hipStreamSynchronize(t->stream));
  } catch (HipErr& h) {
    t->err = h.msg;
    return (int)CYC_ERR_HIP;
  } catch (std::bad_alloc&) {
    t->err = "host allocation failed";
    return (int)CYC_ERR_OOM;
  }
  return (int)CYC_OK;
}

// ---------------------------------------------------------------- whole-table counts and comparison
// Failures of the table entry points land in cyc_table_error(t), as cyc_table_cells' do.
static int table_guarded(cyc_table* t, const std::function<int()>& f) {
  try {
    return f();
  } catch (HipErr& h) {
    t->err = h.msg;
    return (int)CYC_ERR_HIP;
  } catch (std::bad_alloc&) {
    t->err = "host allocation failed";
    return (int)CYC_ERR_OOM;
  }
}

static bool table_whole(const cyc_table* t) {
  return t->partition == CYC_ROWS_SOURCE || (t->row_lo == 0 && t->row_hi == int64_t(t->P));
}

// The tile kernel's view of a whole target-row table (sources [0, P)) or of a source-row table.
static TileArgs tile_args(const cyc_table* t, int64_t k_lo, int64_t k_hi) {
  TileArgs a{};
  a.P = t->P, a.K = t->K, a.W = t->W;
  a.WA = t->wa, a.w0 = t->w0;
  a.s_lo = uint32_t(t->row_lo), a.s_hi = uint32_t(t->row_hi);
  a.k_lo = uint32_t(k_lo), a.nk = uint32_t(k_hi - k_lo);
  a.a = TablePlanes{t->in, t->eg, t->status};
  return a;
}

static dim3 tile_grid(const cyc_table* t, uint32_t source_words = TT_WORDS) {
  return dim3((t->W + TT_WORDS - 1) / TT_WORDS, (t->wa + source_words - 1) / source_words);
}

int cyc_table_counts(cyc_table* t, int64_t k_lo, int64_t k_hi, int64_t* ingress, int64_t* egress, int64_t* combined,
                     int64_t* no_job) {
  if (!t) return CYC_ERR_ARG;
  auto bad = [&](const char* m) {
    t->err = m;
    return (int)CYC_ERR_ARG;
  };
  if (k_lo < 0 || k_hi > int64_t(t->K) || k_lo > k_hi) return bad("slot range out of bounds");
  if (!ingress && !egress && !combined && !no_job) return bad("no output requested");
  const bool whole = table_whole(t);
  // a partial target-row table holds the ingress rows of its destinations and the egress rows of its
  // sources: no cell has both
  if (!whole && (combined || no_job)) return bad("ingress cells need destinations inside the table's rows");
  const int64_t nk = k_hi - k_lo, P = t->P, K = t->K, rows = t->row_hi - t->row_lo;
  for (int64_t i = 0; i < nk * 6; i++) {
    if (ingress) ingress[i] = 0;
    if (egress) egress[i] = 0;
    if (combined) combined[i] = 0;
  }
  if (no_job) *no_job = 0;
  if (!nk || !P) return (int)CYC_OK;
  return table_guarded(t, [&]() -> int {
    DeviceGuard dg(t->device);
    if (!t->stream) HIPCHK(hipStreamCreateWithFlags(&t->stream, hipStreamNonBlocking));
    // allowed cells per (row, slot): whole tables [nk][3][P] by destination (Ingress, Egress, Combined);
    // partial ones [rows][nk][2] (Ingress of destination row r, Egress of source row r)
    const int per = whole ? 3 : 2;
    const uint64_t n_cnt = uint64_t(whole ? P : rows) * nk * per;
    std::vector<unsigned long long> cnt(n_cnt, 0);
    std::vector<uint8_t> st(size_t(P) * K);
    DevBuf d_cnt, d_valid;
    if (n_cnt) {
      d_cnt.alloc(n_cnt * 8);
      HIPCHK(hipMemsetAsync(d_cnt.p, 0, n_cnt * 8, t->stream));
    }
    if (whole && rows) {
      TileArgs a = tile_args(t, k_lo, k_hi);
      a.cnt = d_cnt.as<unsigned long long>();
      k_table_tiles<false><<<tile_grid(t), 1024, 0, t->stream>>>(a);
      HIPCHK(hipGetLastError());
    } else if (rows) {
      RowCountArgs a{};
      a.P = t->P, a.K = t->K, a.W = t->W, a.row_lo = uint32_t(t->row_lo), a.rows = uint32_t(rows);
      a.k_lo = uint32_t(k_lo), a.nk = uint32_t(nk);
      a.t = TablePlanes{t->in, t->eg, t->status};
      d_valid.alloc(uint64_t(nk) * t->W * 8);
      a.valid = d_valid.as<uint64_t>();
      a.cnt = d_cnt.as<unsigned long long>();
      k_table_valid_words<<<grid1(uint64_t(nk) * t->W, 256), 256, 0, t->stream>>>(a);
      HIPCHK(hipGetLastError());
      k_table_row_counts<<<unsigned((uint64_t(rows) * nk + 3) / 4), 256, 0, t->stream>>>(a);
      HIPCHK(hipGetLastError());
    }
    if (n_cnt) HIPCHK(hipMemcpyAsync(cnt.data(), d_cnt.p, n_cnt * 8, hipMemcpyDeviceToHost, t->stream));
    HIPCHK(hipMemcpyAsync(st.data(), t->status, st.size(), hipMemcpyDeviceToHost, t->stream));
    HIPCHK(hipStreamSynchronize(t->stream));
    // the status-only terms (jobrunner.go:36-55): a BadPortProtocol / BadNamedPort job is one code for
    // every source of the destination, Egress unknown; a slot without a job is CYC_CONN_NO_JOB
    const int64_t n_src = whole ? rows : P;  // sources of an ingress row's cells
    for (int64_t kk = 0; kk < nk; kk++) {
      int64_t* oi = ingress ? ingress + kk * 6 : nullptr;
      int64_t* oe = egress ? egress + kk * 6 : nullptr;
      int64_t* oc = combined ? combined + kk * 6 : nullptr;
      // ingress (and combined) over the destinations the table answers; egress over every destination
      for (int64_t d = 0; d < P; d++) {
        const uint8_t s = st[size_t(d * K + k_lo + kk)];
        const bool in_rows = whole || (d >= t->row_lo && d < t->row_hi);
        const int inv = s == CYC_JOB_BAD_PORT_PROTOCOL ? CYC_CONN_INVALID_PORT_PROTOCOL : CYC_CONN_INVALID_NAMED_PORT;
        if (s == CYC_JOB_VALID) {
          if (whole) {
            const unsigned long long* c = &cnt[size_t(kk * 3 * P + d)];
            if (oi) oi[CYC_CONN_ALLOWED] += int64_t(c[0]), oi[CYC_CONN_BLOCKED] += rows - int64_t(c[0]);
            if (oe) oe[CYC_CONN_ALLOWED] += int64_t(c[P]), oe[CYC_CONN_BLOCKED] += rows - int64_t(c[P]);
            if (oc) oc[CYC_CONN_ALLOWED] += int64_t(c[2 * P]), oc[CYC_CONN_BLOCKED] += rows - int64_t(c[2 * P]);
          } else {
            if (oi && in_rows) {
              const int64_t c = int64_t(cnt[size_t(((d - t->row_lo) * nk + kk) * 2)]);
              oi[CYC_CONN_ALLOWED] += c, oi[CYC_CONN_BLOCKED] += n_src - c;
            }
            if (oe) oe[CYC_CONN_BLOCKED] += rows;  // (the allowed ones move over below)
          }
        } else if (s == CYC_JOB_NONE) {
          if (no_job) *no_job += rows;
        } else {
          if (oi && in_rows) oi[inv] += n_src;
          if (oc) oc[inv] += rows;
          if (oe) oe[CYC_CONN_UNKNOWN] += rows;
        }
      }
      if (!whole && oe)
        for (int64_t r = 0; r < rows; r++) {
          const int64_t c = int64_t(cnt[size_t((r * nk + kk) * 2 + 1)]);
          oe[CYC_CONN_ALLOWED] += c, oe[CYC_CONN_BLOCKED] -= c;
        }
    }
    return (int)CYC_OK;
  });
}

int cyc_table_pod_counts(cyc_table* t, int view, int64_t k_lo, int64_t k_hi, int64_t* by_src, int64_t* by_dst) {
  if (!t) return CYC_ERR_ARG;
  auto bad = [&](const char* m) {
    t->err = m;
    return (int)CYC_ERR_ARG;
  };
  if (view != CYC_VIEW_INGRESS && view != CYC_VIEW_EGRESS && view != CYC_VIEW_COMBINED) return bad("unknown view");
  if (k_lo < 0 || k_hi > int64_t(t->K) || k_lo > k_hi) return bad("slot range out of bounds");
  if (!by_src && !by_dst) return bad("no output requested");
  if (!table_whole(t)) return bad("ingress cells need destinations inside the table's rows");
  const int64_t nk = k_hi - k_lo, P = t->P, K = t->K, rows = t->row_hi - t->row_lo;
  if (!nk || !P) return (int)CYC_OK;
  return table_guarded(t, [&]() -> int {
    DeviceGuard dg(t->device);
    if (!t->stream) HIPCHK(hipStreamCreateWithFlags(&t->stream, hipStreamNonBlocking));
    // allowed cells per (slot, destination) of the three views (cyc_table_counts), and with by_src per (slot,
    // source) of `view`
    const int64_t src_stride = int64_t(t->wa) * 64;  // (TileArgs::src_cnt: source-minor)
    const uint64_t n_cnt = uint64_t(nk) * 3 * P, n_src = by_src ? uint64_t(nk) * src_stride : 0;
    std::vector<unsigned long long> cnt(n_cnt, 0), src(n_src, 0);
    std::vector<uint8_t> st(size_t(P) * K);
    DevBuf d_cnt;
    if (rows) {
      d_cnt.alloc((n_cnt + n_src) * 8);
      HIPCHK(hipMemsetAsync(d_cnt.p, 0, (n_cnt + n_src) * 8, t->stream));
      TileArgs a = tile_args(t, k_lo, k_hi);
      a.cnt = d_cnt.as<unsigned long long>();
      a.src_cnt = a.cnt + n_cnt;
      a.view = uint32_t(view);
      if (by_src) k_table_tiles<false, true><<<tile_grid(t), 1024, 0, t->stream>>>(a);
      else k_table_tiles<false><<<tile_grid(t), 1024, 0, t->stream>>>(a);
      HIPCHK(hipGetLastError());
      HIPCHK(hipMemcpyAsync(cnt.data(), a.cnt, n_cnt * 8, hipMemcpyDeviceToHost, t->stream));
      if (n_src) HIPCHK(hipMemcpyAsync(src.data(), a.src_cnt, n_src * 8, hipMemcpyDeviceToHost, t->stream));
    }
    HIPCHK(hipMemcpyAsync(st.data(), t->status, st.size(), hipMemcpyDeviceToHost, t->stream));
    HIPCHK(hipStreamSynchronize(t->stream));
    // the status-only terms, as cyc_table_counts': the code of a destination's slot that is not VALID holds for
    // every source, so a source's row has as many cells of it as there are such destinations
    const int inv_np = view == CYC_VIEW_EGRESS ? CYC_CONN_UNKNOWN : CYC_CONN_INVALID_NAMED_PORT;
    const int inv_pp = view == CYC_VIEW_EGRESS ? CYC_CONN_UNKNOWN : CYC_CONN_INVALID_PORT_PROTOCOL;
    for (int64_t kk = 0; kk < nk; kk++) {
      int64_t n_of[4] = {0, 0, 0, 0};  // destinations per cyc_job_status
      for (int64_t d = 0; d < P; d++) {
        const uint8_t s = st[size_t(d * K + k_lo + kk)];
        n_of[s <= CYC_JOB_BAD_PORT_PROTOCOL ? s : CYC_JOB_BAD_NAMED_PORT]++;  // (any other value: as cyc_table_counts)
        if (!by_dst) continue;
        int64_t* o = by_dst + (d * nk + kk) * CYC_POD_CODES;
        for (int c = 0; c < CYC_POD_CODES; c++) o[c] = 0;
        if (s == CYC_JOB_VALID) {
          const int64_t a = int64_t(cnt[size_t((kk * 3 + view) * P + d)]);
          o[CYC_CONN_ALLOWED] = a, o[CYC_CONN_BLOCKED] = rows - a;
        } else {
          o[s == CYC_JOB_NONE ? 6 : s == CYC_JOB_BAD_PORT_PROTOCOL ? inv_pp : inv_np] = rows;
        }
      }
      for (int64_t i = 0; by_src && i < rows; i++) {
        int64_t* o = by_src + (i * nk + kk) * CYC_POD_CODES;
        for (int c = 0; c < CYC_POD_CODES; c++) o[c] = 0;
        const int64_t a = int64_t(src[size_t(kk * src_stride + i)]);
        o[CYC_CONN_ALLOWED] = a, o[CYC_CONN_BLOCKED] = n_of[CYC_JOB_VALID] - a;
        o[inv_np] += n_of[CYC_JOB_BAD_NAMED_PORT], o[inv_pp] += n_of[CYC_JOB_BAD_PORT_PROTOCOL];
        o[6] = n_of[CYC_JOB_NONE];
      }
    }
    return (int)CYC_OK;
  });
}

// What cyc_table_compare and cyc_table_pod_compare check alike; nullptr when the arguments are fine.
static const char* compare_args_bad(const cyc_table* ta, const cyc_table* tb, int64_t k_lo, int64_t k_hi) {
  if (!tb) return "null table";
  if (ta->device != tb->device || ta->P != tb->P || ta->K != tb->K || ta->partition != tb->partition ||
      ta->row_lo != tb->row_lo || ta->row_hi != tb->row_hi)
    return "cannot compare tables of different devices, shapes, partitions or rows";
  if (k_lo < 0 || k_hi > int64_t(ta->K) || k_lo > k_hi) return "slot range out of bounds";
  if (!table_whole(ta)) return "ingress cells need destinations inside the table's rows";
  return nullptr;
}

// The compare pass over the tiles and what the host needs of it: the kernel's per-destination buffer (TileArgs::cnt),
// with `src` its per-source buffer (TileArgs::src_cnt) too, and a's status plane.  Zeros where the table has no cell.
struct CompareTiles {
  std::vector<unsigned long long> cnt, src;
  std::vector<uint8_t> sa;
};
static CompareTiles compare_tiles(cyc_table* t, cyc_table* tb, int64_t k_lo, int64_t k_hi, int ignore_loopback, uint64_t* d_diff,
                                  bool src) {
  const uint64_t nk = uint64_t(k_hi - k_lo), P = t->P, n_cnt = P * (nk + 2), n_src = src ? (nk + 1) * t->wa * 64 : 0;
  CompareTiles r;
  r.cnt.assign(n_cnt, 0), r.src.assign(n_src, 0), r.sa.assign(size_t(P) * t->K, 0);
  if (!P || t->row_hi == t->row_lo) return r;
  if (!t->stream) HIPCHK(hipStreamCreateWithFlags(&t->stream, hipStreamNonBlocking));
  DevBuf d_cnt;
  d_cnt.alloc((n_cnt + n_src) * 8);
  HIPCHK(hipMemsetAsync(d_cnt.p, 0, (n_cnt + n_src) * 8, t->stream));
  TileArgs a = tile_args(t, k_lo, k_hi);
  a.b = TablePlanes{tb->in, tb->eg, tb->status};
  a.ignore_loopback = ignore_loopback ? 1u : 0u;
  a.cnt = d_cnt.as<unsigned long long>();
  a.src_cnt = a.cnt + n_cnt;
  a.diff = d_diff;
  if (src) k_table_tiles<true, true><<<tile_grid(t, tile_source_words(true, true)), 1024, 0, t->stream>>>(a);
  else k_table_tiles<true><<<tile_grid(t), 1024, 0, t->stream>>>(a);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(r.cnt.data(), a.cnt, n_cnt * 8, hipMemcpyDeviceToHost, t->stream));
  if (n_src) HIPCHK(hipMemcpyAsync(r.src.data(), a.src_cnt, n_src * 8, hipMemcpyDeviceToHost, t->stream));
  HIPCHK(hipMemcpyAsync(r.sa.data(), t->status, r.sa.size(), hipMemcpyDeviceToHost, t->stream));
  HIPCHK(hipStreamSynchronize(t->stream));  // (d_cnt is freed after it)
  return r;
}

// per job (ValueCountsByProtocol :89-107, ResultsByProtocol :14-20,69-79): every cell whose job a holds, summed
// (slot_counts) and per destination (dst_counts), each optional
static void compare_jobs_by_dst(const cyc_table* t, const CompareTiles& r, int64_t k_lo, int64_t nk, int ignore_loopback,
                                int64_t* slot_counts, int64_t* dst_counts) {
  const int64_t P = t->P, K = t->K, rows = t->row_hi - t->row_lo;
  for (int64_t i = 0; slot_counts && i < nk * 3; i++) slot_counts[i] = 0;
  if (slot_counts || dst_counts)
    for (int64_t d = 0; d < P; d++)
      for (int64_t kk = 0; kk < nk; kk++) {
        int64_t v[3] = {0, 0, 0};
        if (r.sa[size_t(d * K + k_lo + kk)] != CYC_JOB_NONE) {
          v[2] = ignore_loopback && d >= t->row_lo && d < t->row_hi ? 1 : 0;
          v[1] = int64_t(r.cnt[size_t(kk * P + d)]);
          v[0] = rows - v[1] - v[2];
        }
        for (int x = 0; x < 3; x++) {
          if (slot_counts) slot_counts[kk * 3 + x] += v[x];
          if (dst_counts) dst_counts[(d * nk + kk) * 3 + x] = v[x];
        }
      }
}

int cyc_table_compare(cyc_table* ta, cyc_table* tb, int64_t k_lo, int64_t k_hi, int ignore_loopback, int64_t pair_counts[3],
                      int64_t* slot_counts, int64_t* dst_counts, uint64_t* d_diff) {
  if (!ta) return CYC_ERR_ARG;
  cyc_table* t = ta;
  auto bad = [&](const char* m) {
    t->err = m;
    return (int)CYC_ERR_ARG;
  };
  if (!tb) return bad("null table");
  if (!pair_counts) return bad("null pair_counts");
  if (const char* why = compare_args_bad(ta, tb, k_lo, k_hi)) return bad(why);
  if (reinterpret_cast<uintptr_t>(d_diff) % 8) return bad("d_diff is not 8-byte aligned");
  const int64_t nk = k_hi - k_lo, P = t->P, rows = t->row_hi - t->row_lo;
  return table_guarded(t, [&]() -> int {
    DeviceGuard dg(t->device);
    const CompareTiles r = compare_tiles(t, tb, k_lo, k_hi, ignore_loopback, d_diff, false);
    const std::vector<unsigned long long>& cnt = r.cnt;
    // ValueCounts (comparisontable.go:109-123): a pair is the Items' equalsDict (:26-36) unless it is an
    // ignored loopback; the table answers the pairs (s in its rows, every d)
    int64_t differ = 0, self_differ = 0;
    for (int64_t d = 0; d < P; d++) differ += int64_t(cnt[size_t(nk * P + d)]), self_differ += int64_t(cnt[size_t((nk + 1) * P + d)]);
    pair_counts[2] = ignore_loopback ? rows : 0;
    pair_counts[1] = differ - (ignore_loopback ? self_differ : 0);
    pair_counts[0] = rows * P - pair_counts[1] - pair_counts[2];
    compare_jobs_by_dst(t, r, k_lo, nk, ignore_loopback, slot_counts, dst_counts);
    return (int)CYC_OK;
  });
}

int cyc_table_pod_compare(cyc_table* ta, cyc_table* tb, int64_t k_lo, int64_t k_hi, int ignore_loopback, int64_t* src_pairs,
                          int64_t* dst_pairs, int64_t* src_slots, int64_t* dst_slots) {
  if (!ta) return CYC_ERR_ARG;
  cyc_table* t = ta;
  auto bad = [&](const char* m) {
    t->err = m;
    return (int)CYC_ERR_ARG;
  };
  if (const char* why = compare_args_bad(ta, tb, k_lo, k_hi)) return bad(why);
  if (!src_pairs && !dst_pairs && !src_slots && !dst_slots) return bad("no output requested");
  const int64_t nk = k_hi - k_lo, P = t->P, K = t->K, rows = t->row_hi - t->row_lo, il = ignore_loopback ? 1 : 0;
  return table_guarded(t, [&]() -> int {
    DeviceGuard dg(t->device);
    const CompareTiles r = compare_tiles(t, tb, k_lo, k_hi, ignore_loopback, nullptr, src_pairs || src_slots);
    const unsigned long long* self = r.cnt.data() + (nk + 1) * P;  // whether the pair (d, d) differs
    // the pairs (ValueCounts, as cyc_table_compare): of destination d over the table's sources, of source s over
    // every destination; the loopback pair is ignored whether it differs or not
    for (int64_t d = 0; dst_pairs && d < P; d++) {
      int64_t* o = dst_pairs + d * 3;
      o[2] = il && d >= t->row_lo && d < t->row_hi ? 1 : 0;
      o[1] = int64_t(r.cnt[size_t(nk * P + d)]) - (il ? int64_t(self[d]) : 0);
      o[0] = rows - o[1] - o[2];
    }
    const int64_t src_stride = int64_t(t->wa) * 64;  // (TileArgs::src_cnt: source-minor)
    for (int64_t i = 0; src_pairs && i < rows; i++) {
      int64_t* o = src_pairs + i * 3;
      o[2] = il;
      o[1] = int64_t(r.src[size_t(nk * src_stride + i)]) - (il ? int64_t(self[t->row_lo + i]) : 0);
      o[0] = P - o[1] - o[2];
    }
    compare_jobs_by_dst(t, r, k_lo, nk, ignore_loopback, nullptr, dst_slots);
    // per job and source: a's jobs of slot kk are the destinations whose status is not NONE, the loopback cell is
    // ignored when (s, kk) is a job of a
    for (int64_t kk = 0; src_slots && kk < nk; kk++) {
      int64_t jobs = 0;
      for (int64_t d = 0; d < P; d++) jobs += r.sa[size_t(d * K + k_lo + kk)] != CYC_JOB_NONE;
      for (int64_t i = 0; i < rows; i++) {
        int64_t* o = src_slots + (i * nk + kk) * 3;
        o[2] = il && r.sa[size_t((t->row_lo + i) * K + k_lo + kk)] != CYC_JOB_NONE ? 1 : 0;
        o[1] = int64_t(r.src[size_t(kk * src_stride + i)]);
        o[0] = jobs - o[1] - o[2];
      }
    }
    return (int)CYC_OK;
  });
}

// ---------------------------------------------------------------- counts and comparison per pod-group pair
constexpr int64_t GROUP_CELLS_MAX = int64_t(1) << 27;  // n_groups^2 * slots of one call

// The checks the two group entry points share; nullptr when the arguments are fine.
static const char* group_args_bad(const cyc_table* t, const int32_t* group_of, int64_t G, int64_t k_lo, int64_t k_hi, std::string& why) {
  if (!group_of) return "null group_of";
  if (k_lo < 0 || k_hi > int64_t(t->K) || k_lo > k_hi) return "slot range out of bounds";
  if (G < 1) return "n_groups must be at least 1";
  if (G > GROUP_CELLS_MAX || G * G * std::max<int64_t>(k_hi - k_lo, 1) > GROUP_CELLS_MAX)
    return "n_groups^2 * slots exceeds the limit of 134217728 (2^27)";
  for (int64_t p = 0; p < int64_t(t->P); p++)
    if (group_of[p] < -1 || group_of[p] >= G) {
      why = "group_of[" + std::to_string(p) + "] = " + std::to_string(group_of[p]) + " is neither -1 nor a group in [0, " +
            std::to_string(G) + ")";
      return why.c_str();
    }
  return nullptr;
}

// What k_table_group_tiles takes of a grouping (GroupArgs, dev_table.hpp), from one walk over the pods: the
// (group, mask) entries of every source word of the table in pod order, the groups of every block row of 16
// source words and block column of 1024 destinations numbered in order of appearance, and the group sizes
// for the host-side terms.
extern "C++" {
struct GroupTables {
  std::vector<uint32_t> ent_ptr{0}, ent_grp, ent_loc, row_ptr, row_grp, dst_loc, col_ptr, col_grp;
  std::vector<uint64_t> ent_mask;
  std::vector<int64_t> n_src, n_dst;  // pods of a group among the table's sources, among all destinations
  DevBuf dev[10];

  GroupTables(const cyc_table* t, const int32_t* group_of, int64_t G) : n_src(size_t(G), 0), n_dst(size_t(G), 0) {
    constexpr uint32_t NONE = ~0u;
    const size_t n = size_t(G);
    std::vector<uint32_t> word_of(n, NONE), ent_of(n), blk_of(n, NONE), loc_of(n);
    for (uint32_t j = 0; j < t->wa; j++) {
      if (j % TT_WORDS == 0) row_ptr.push_back(uint32_t(row_grp.size()));
      for (uint32_t b = 0; b < 64; b++) {
        const int64_t s = int64_t(t->w0 + j) * 64 + b;
        if (s < t->row_lo || s >= t->row_hi || group_of[s] < 0) continue;
        const uint32_t g = uint32_t(group_of[s]);
        n_src[g]++;
        if (word_of[g] != j) {
          if (blk_of[g] != j / TT_WORDS) {
            blk_of[g] = j / TT_WORDS, loc_of[g] = uint32_t(row_grp.size()) - row_ptr.back();
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
    dst_loc.assign(t->P, 0);
    for (uint32_t d = 0; d < t->P; d++) {
      if (d % (TT_WORDS * 64) == 0) col_ptr.push_back(uint32_t(col_grp.size()));
      if (group_of[d] < 0) continue;
      const uint32_t g = uint32_t(group_of[d]);
      n_dst[g]++;
      if (blk_of[g] != d / (TT_WORDS * 64)) {
        blk_of[g] = d / (TT_WORDS * 64), loc_of[g] = uint32_t(col_grp.size()) - col_ptr.back();
        col_grp.push_back(g);
      }
      dst_loc[d] = loc_of[g];
    }
    col_ptr.push_back(uint32_t(col_grp.size()));
  }

  // (asynchronous: the vectors live until the caller has synchronised the stream)
  template <class T>
  const T* put(int i, const T* v, size_t n, hipStream_t st) {
    dev[i].alloc(std::max<size_t>(n * sizeof(T), 16));
    if (n) HIPCHK(hipMemcpyAsync(dev[i].p, v, n * sizeof(T), hipMemcpyHostToDevice, st));
    return dev[i].as<T>();
  }
  GroupArgs args(const TileArgs& tile, const int32_t* group_of, int64_t G, hipStream_t st) {
    GroupArgs g{};
    g.t = tile, g.G = uint32_t(G);
    g.ent_ptr = put(0, ent_ptr.data(), ent_ptr.size(), st);
    g.ent_mask = put(1, ent_mask.data(), ent_mask.size(), st);
    g.ent_grp = put(2, ent_grp.data(), ent_grp.size(), st);
    g.ent_loc = put(3, ent_loc.data(), ent_loc.size(), st);
    g.row_ptr = put(4, row_ptr.data(), row_ptr.size(), st);
    g.row_grp = put(5, row_grp.data(), row_grp.size(), st);
    g.dst_grp = put(6, group_of, tile.P, st);
    g.dst_loc = put(7, dst_loc.data(), dst_loc.size(), st);
    g.col_ptr = put(8, col_ptr.data(), col_ptr.size(), st);
    g.col_grp = put(9, col_grp.data(), col_grp.size(), st);
    return g;
  }
};
}  // extern "C++"

int cyc_table_group_counts(cyc_table* t, const int32_t* group_of, int64_t n_groups, int64_t k_lo, int64_t k_hi, int64_t* ingress,
                           int64_t* egress, int64_t* combined, int64_t* no_job) {
  if (!t) return CYC_ERR_ARG;
  auto bad = [&](const std::string& m) {
    t->err = m;
    return (int)CYC_ERR_ARG;
  };
  std::string why;
  if (const char* m = group_args_bad(t, group_of, n_groups, k_lo, k_hi, why)) return bad(m);
  if (!ingress && !egress && !combined && !no_job) return bad("no output requested");
  if (!table_whole(t)) return bad("ingress cells need destinations inside the table's rows");
  const int64_t nk = k_hi - k_lo, P = t->P, K = t->K, G = n_groups, GG = G * G, rows = t->row_hi - t->row_lo;
  int64_t* out[3] = {ingress, egress, combined};
  for (int x = 0; x < 3; x++)
    if (out[x]) std::fill(out[x], out[x] + GG * nk * 6, int64_t(0));
  if (no_job) std::fill(no_job, no_job + GG, int64_t(0));
  if (!nk || !P) return (int)CYC_OK;
  return table_guarded(t, [&]() -> int {
    DeviceGuard dg(t->device);
    if (!t->stream) HIPCHK(hipStreamCreateWithFlags(&t->stream, hipStreamNonBlocking));
    // allowed cells [nk][3][G][G] of Ingress, Egress, Combined
    const uint64_t n_cnt = uint64_t(nk) * 3 * GG;
    std::vector<unsigned long long> cnt(n_cnt, 0);
    std::vector<uint8_t> st(size_t(P) * K);
    GroupTables gt(t, group_of, G);
    DevBuf d_cnt;
    if (rows) {
      d_cnt.alloc(n_cnt * 8);
      HIPCHK(hipMemsetAsync(d_cnt.p, 0, n_cnt * 8, t->stream));
      GroupArgs a = gt.args(tile_args(t, k_lo, k_hi), group_of, G, t->stream);
      a.t.cnt = d_cnt.as<unsigned long long>();
      k_table_group_tiles<false><<<tile_grid(t), 1024, 0, t->stream>>>(a);
      HIPCHK(hipGetLastError());
      HIPCHK(hipMemcpyAsync(cnt.data(), d_cnt.p, n_cnt * 8, hipMemcpyDeviceToHost, t->stream));
    }
    HIPCHK(hipMemcpyAsync(st.data(), t->status, st.size(), hipMemcpyDeviceToHost, t->stream));
    HIPCHK(hipStreamSynchronize(t->stream));
    // the status-only terms, as cyc_table_counts': per (destination group, slot) the destinations of each
    // status, times the sources of the source group
    std::vector<int64_t> by_status(size_t(G) * nk * 4, 0);  // [gd][kk][cyc_job_status]
    for (int64_t d = 0; d < P; d++)
      if (group_of[d] >= 0)
        for (int64_t kk = 0; kk < nk; kk++) by_status[size_t((group_of[d] * nk + kk) * 4 + (st[size_t(d * K + k_lo + kk)] & 3))]++;
    for (int64_t gs = 0; gs < G; gs++) {
      const int64_t ns = gt.n_src[size_t(gs)];
      if (!ns) continue;
      for (int64_t gd = 0; gd < G; gd++) {
        if (!gt.n_dst[size_t(gd)]) continue;
        for (int64_t kk = 0; kk < nk; kk++) {
          const int64_t* s = &by_status[size_t((gd * nk + kk) * 4)];
          const int64_t valid = ns * s[CYC_JOB_VALID], bpp = ns * s[CYC_JOB_BAD_PORT_PROTOCOL], bnp = ns * s[CYC_JOB_BAD_NAMED_PORT];
          const size_t at = size_t(((gs * G + gd) * nk + kk) * 6);
          for (int x = 0; x < 3; x++) {
            if (!out[x]) continue;
            const int64_t allowed = int64_t(cnt[size_t((kk * 3 + x) * GG + gs * G + gd)]);
            int64_t* o = out[x] + at;
            o[CYC_CONN_ALLOWED] = allowed, o[CYC_CONN_BLOCKED] = valid - allowed;
            if (x == 1) o[CYC_CONN_UNKNOWN] = bpp + bnp;
            else o[CYC_CONN_INVALID_PORT_PROTOCOL] = bpp, o[CYC_CONN_INVALID_NAMED_PORT] = bnp;
          }
          if (no_job) no_job[gs * G + gd] += ns * s[CYC_JOB_NONE];
        }
      }
    }
    return (int)CYC_OK;
  });
}

int cyc_table_group_compare(cyc_table* ta, cyc_table* tb, const int32_t* group_of, int64_t n_groups, int64_t k_lo, int64_t k_hi,
                            int ignore_loopback, int64_t* pair_counts, int64_t* slot_counts) {
  if (!ta) return CYC_ERR_ARG;
  cyc_table* t = ta;
  auto bad = [&](const std::string& m) {
    t->err = m;
    return (int)CYC_ERR_ARG;
  };
  if (!tb) return bad("null table");
  if (!pair_counts) return bad("no output requested");
  if (ta->device != tb->device || ta->P != tb->P || ta->K != tb->K || ta->partition != tb->partition ||
      ta->row_lo != tb->row_lo || ta->row_hi != tb->row_hi)
    return bad("cannot compare tables of different devices, shapes, partitions or rows");
  std::string why;
  if (const char* m = group_args_bad(t, group_of, n_groups, k_lo, k_hi, why)) return bad(m);
  if (!table_whole(t)) return bad("ingress cells need destinations inside the table's rows");
  const int64_t nk = k_hi - k_lo, P = t->P, K = t->K, G = n_groups, GG = G * G, rows = t->row_hi - t->row_lo;
  std::fill(pair_counts, pair_counts + GG * 3, int64_t(0));
  if (slot_counts) std::fill(slot_counts, slot_counts + GG * nk * 3, int64_t(0));
  if (!P) return (int)CYC_OK;
  return table_guarded(t, [&]() -> int {
    DeviceGuard dg(t->device);
    if (!t->stream) HIPCHK(hipStreamCreateWithFlags(&t->stream, hipStreamNonBlocking));
    // [nk + 1][G][G]: differing cells per slot, then the differing pairs; then [G]: differing pairs (d, d)
    const uint64_t n_cnt = uint64_t(nk + 1) * GG + G;
    std::vector<unsigned long long> cnt(n_cnt, 0);
    std::vector<uint8_t> sa(size_t(P) * K);
    GroupTables gt(t, group_of, G);
    if (rows) {
      DevBuf d_cnt;
      d_cnt.alloc(n_cnt * 8);
      HIPCHK(hipMemsetAsync(d_cnt.p, 0, n_cnt * 8, t->stream));
      GroupArgs a = gt.args(tile_args(t, k_lo, k_hi), group_of, G, t->stream);
      a.t.b = TablePlanes{tb->in, tb->eg, tb->status};
      a.t.ignore_loopback = ignore_loopback ? 1u : 0u;
      a.t.cnt = d_cnt.as<unsigned long long>();
      k_table_group_tiles<true><<<tile_grid(t), 1024, 0, t->stream>>>(a);
      HIPCHK(hipGetLastError());
      HIPCHK(hipMemcpyAsync(cnt.data(), d_cnt.p, n_cnt * 8, hipMemcpyDeviceToHost, t->stream));
      HIPCHK(hipMemcpyAsync(sa.data(), ta->status, sa.size(), hipMemcpyDeviceToHost, t->stream));
      HIPCHK(hipStreamSynchronize(t->stream));  // (d_cnt is freed after it)
    }
    // the terms of cyc_table_compare, per group pair: jobs[gd][kk] = destinations of the group where a holds a
    // job, loop[g][kk] = those among the table's sources (the loopback cells)
    std::vector<int64_t> jobs(size_t(G) * nk, 0), loop(size_t(G) * nk, 0);
    if (rows)
      for (int64_t d = 0; d < P; d++)
        if (group_of[d] >= 0)
          for (int64_t kk = 0; kk < nk; kk++)
            if (sa[size_t(d * K + k_lo + kk)] != CYC_JOB_NONE) {
              jobs[size_t(group_of[d] * nk + kk)]++;
              if (ignore_loopback && d >= t->row_lo && d < t->row_hi) loop[size_t(group_of[d] * nk + kk)]++;
            }
    for (int64_t gs = 0; gs < G; gs++) {
      const int64_t ns = gt.n_src[size_t(gs)];
      if (!ns) continue;
      for (int64_t gd = 0; gd < G; gd++) {
        const int64_t self = gs == gd ? 1 : 0;
        int64_t* p = pair_counts + (gs * G + gd) * 3;
        p[2] = ignore_loopback ? self * ns : 0;
        p[1] = int64_t(cnt[size_t(nk * GG + gs * G + gd)]) - (ignore_loopback ? self * int64_t(cnt[size_t((nk + 1) * GG + gs)]) : 0);
        p[0] = ns * gt.n_dst[size_t(gd)] - p[1] - p[2];
        for (int64_t kk = 0; slot_counts && kk < nk; kk++) {
          int64_t* v = slot_counts + ((gs * G + gd) * nk + kk) * 3;
          v[2] = self * loop[size_t(gs * nk + kk)];
          v[1] = int64_t(cnt[size_t(kk * GG + gs * G + gd)]);
          v[0] = ns * jobs[size_t(gd * nk + kk)] - v[1] - v[2];
        }
      }
    }
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
  auto bad = [&](const std::string& m) {
    t->err = m;
    return (int)CYC_ERR_ARG;
  };
  if (!n || !s_next || !total) return bad("null n, s_next or total");
  *n = 0, *total = 0, *s_next = s_from;
  if (k_lo < 0 || k_hi > int64_t(t->K) || k_lo > k_hi) return bad("slot range out of bounds");
  if (!table_whole(t)) return bad("ingress cells need destinations inside the table's rows");
  if (s_from < t->row_lo || s_from > t->row_hi) return bad("s_from outside the table's rows");
  if (cap < 0) return bad("negative cap");
  if (!cells && cap > 0) return bad("null cells");
  const bool count_only = !cells;
  const int64_t nk = k_hi - k_lo, rows = t->row_hi - s_from;
  if (!nk && !count_only) *s_next = t->row_hi;
  if (!nk || !rows) return (int)CYC_OK;
  return table_guarded(t, [&]() -> int {
    DeviceGuard dg(t->device);
    if (!t->stream) HIPCHK(hipStreamCreateWithFlags(&t->stream, hipStreamNonBlocking));
    const bool cmp = tb != nullptr;
    FindArgs a{};
    a.t = tile_args(t, k_lo, k_hi);
    if (cmp) a.t.b = TablePlanes{tb->in, tb->eg, tb->status};
    a.t.ignore_loopback = ignore_loopback ? 1u : 0u;
    a.view = uint32_t(view), a.code_mask = code_mask;
    a.NB = (t->W + TT_WORDS - 1) / TT_WORDS;
    a.bx0 = uint32_t((s_from / 64 - t->w0) / TT_WORDS);
    // ---- pass 1: matches per (destination block, source), then per source
    const uint64_t n_src = uint64_t(t->row_hi - t->row_lo), n_stw = uint64_t(nk) * t->W * 2, n_blk = uint64_t(a.NB) * n_src;
    DevBuf d_cnt, d_stw, d_blk;
    d_cnt.alloc(n_src * 8), d_stw.alloc(n_stw * 8), d_blk.alloc(n_blk * 8);
    HIPCHK(hipMemsetAsync(d_cnt.p, 0, n_src * 8, t->stream));  // (the sources before pass 1's first block)
    a.n_src = uint32_t(n_src);
    a.t.cnt = d_cnt.as<unsigned long long>();
    a.stw = d_stw.as<uint64_t>();
    a.blk = d_blk.as<unsigned long long>();
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
    std::vector<unsigned long long> cnt(n_src);
    HIPCHK(hipMemcpyAsync(cnt.data(), d_cnt.p, n_src * 8, hipMemcpyDeviceToHost, t->stream));
    HIPCHK(hipStreamSynchronize(t->stream));
    // ---- the page: sources [s_from, s_next) are the longest run whose records fit into cap
    const unsigned long long* c = cnt.data() + (s_from - t->row_lo);  // c[i]: source s_from + i
    for (int64_t i = 0; i < rows; i++) *total += int64_t(c[i]);
    if (count_only) return (int)CYC_OK;
    std::vector<unsigned long long> offs(1, 0);  // offs[i]: first record of source s_from + i
    int64_t page = 0;
    while (page < rows && offs.back() + c[page] <= (unsigned long long)cap) offs.push_back(offs.back() + c[page++]);
    if (!page)
      return bad("source " + std::to_string(s_from) + " alone has " + std::to_string(c[0]) + " matching cells, more than cap " +
                 std::to_string(cap));
    *s_next = s_from + page;
    *n = int64_t(offs.back());
    if (!*n) return (int)CYC_OK;
    // ---- pass 2: the records of the page
    DevBuf d_offs, d_out, d_scratch;
    d_offs.alloc(offs.size() * 8), d_out.alloc(uint64_t(*n) * sizeof(cyc_cell));
    HIPCHK(hipMemcpyAsync(d_offs.p, offs.data(), offs.size() * 8, hipMemcpyHostToDevice, t->stream));
    a.s_from = uint32_t(s_from), a.s_next = uint32_t(*s_next);
    a.offs = d_offs.as<unsigned long long>();
    a.out = d_out.as<uint4>();
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

int cyc_table_find(cyc_table* t, int view, uint32_t code_mask, int64_t k_lo, int64_t k_hi, int64_t s_from, cyc_cell* cells, int64_t cap,
                   int64_t* n, int64_t* s_next, int64_t* total) {
  if (!t) return CYC_ERR_ARG;
  if (view != CYC_VIEW_INGRESS && view != CYC_VIEW_EGRESS && view != CYC_VIEW_COMBINED) return t->err = "unknown view", (int)CYC_ERR_ARG;
  if (!code_mask || code_mask >> 6) return t->err = "code_mask must name codes 0..5", (int)CYC_ERR_ARG;
  return table_find(t, nullptr, view, code_mask, 0, k_lo, k_hi, s_from, cells, cap, n, s_next, total);
}

int cyc_table_compare_find(cyc_table* ta, cyc_table* tb, int64_t k_lo, int64_t k_hi, int ignore_loopback, int64_t s_from, cyc_cell* cells,
                           int64_t cap, int64_t* n, int64_t* s_next, int64_t* total) {
  if (!ta) return CYC_ERR_ARG;
  if (!tb) return ta->err = "null table", (int)CYC_ERR_ARG;
  if (ta->device != tb->device || ta->P != tb->P || ta->K != tb->K || ta->partition != tb->partition || ta->row_lo != tb->row_lo ||
      ta->row_hi != tb->row_hi)
    return ta->err = "cannot compare tables of different devices, shapes, partitions or rows", (int)CYC_ERR_ARG;
  return table_find(ta, tb, CYC_VIEW_COMBINED, 0, ignore_loopback, k_lo, k_hi, s_from, cells, cap, n, s_next, total);
}

void cyc_table_destroy(cyc_table* t) {
  if (!t) return;
  DeviceGuard dg(t->device, false);
  if (t->stream) {
    (void)hipStreamSynchronize(t->stream);
    (void)hipStreamDestroy(t->stream);
  }
  delete t;  // owned planes are freed by their DevBufs
}

int cyc_last_timings(cyc_ctx* c, double* ms, int n) {
  if (!c || !ms) return CYC_ERR_ARG;
  if (!c->run.last.timed) return fail(c, CYC_ERR_ARG, c->run.last.ran ? "the last run recorded no timing events (step_events = 0)" : "no run yet");
  return guarded(c, [&] {
    DeviceGuard dg(c->device);
    HIPCHK(hipEventSynchronize(c->run.ev[3]));
    float a = 0, b = 0, r = 0;
    HIPCHK(hipEventElapsedTime(&a, c->run.ev[0], c->run.ev[3]));
    if (!c->run.last.timed_graph) {
      HIPCHK(hipEventElapsedTime(&b, c->run.ev[2], c->run.ev[3]));
      HIPCHK(hipEventElapsedTime(&r, c->run.ev[1], c->run.ev[2]));
      if (c->run.last.phase_used) {  // row phases: phase 2's class rows ran between the emits (ev_p)
        float p2 = 0;
        HIPCHK(hipEventElapsedTime(&p2, c->run.ev_p[0], c->run.ev_p[1]));
        b -= p2;
        r += p2;
      }
    }
    double v[3] = {a, c->run.last.timed_graph ? -1.0 : b, c->run.last.timed_graph ? -1.0 : r};
    for (int i = 0; i < n && i < 3; i++) ms[i] = v[i];
    return (int)CYC_OK;
  });
}

int cyc_last_classes(cyc_ctx* c, int64_t* out, int n) {
  if (!c || !out || n < 2) return CYC_ERR_ARG;
  if (!c->run.last.ran) return fail(c, CYC_ERR_ARG, "no run yet");
  return guarded(c, [&]() -> int {
    DeviceGuard dg(c->device);
    // the last run's stream, not an event recorded after every run: an event at each step's end held
    // the next step's first launch ~4.5 us (config #2: 0.0640 -> 0.0598 ms per step without it, r05at)
    HIPCHK(hipStreamSynchronize(c->run.last.stream));
    for (int d = 0; d < 2; d++) {
      uint32_t v[2] = {0xFFFFFFFFu, 0u};  // reps[]'s head (count - 1) and tail (row phases' phase-2 classes)
      if (c->prep.dir[d].n && c->range.n_act[d]) HIPCHK(hipMemcpy(v, c->prep.dir[d].rep_cnt(), 8, hipMemcpyDeviceToHost));
      out[d] = int64_t(uint32_t(v[0] + 1u)) + int64_t(v[1]);
    }
    return (int)CYC_OK;
  });
}

int cyc_last_emit(cyc_ctx* c, char* name, size_t cap, int64_t* launches) {
  if (!c) return CYC_ERR_ARG;
  if (!c->run.last.ran) return fail(c, CYC_ERR_ARG, "no run yet");
  if (name && cap) {
    const size_t n = std::min(cap - 1, c->run.last.emit_kernel.size());
    std::memcpy(name, c->run.last.emit_kernel.data(), n);
    name[n] = 0;
  }
  if (launches) *launches = c->run.last.emit_launches;
  return CYC_OK;
}

int cyc_set_option(cyc_ctx* c, const char* name, int64_t value) {
  if (!c || !name) return CYC_ERR_ARG;
  std::unique_ptr<DeviceGuard> dg;
  if (c->stream) dg.reset(new DeviceGuard(c->device, false));  // drop_graph may destroy this context's execs
  const std::string n(name);
  return guarded(c, [&]() -> int {
    const OptionRow* o = find_option(name);
    if (!o) return fail(c, CYC_ERR_ARG, "unknown option " + n);
    if (value < o->lo || value > o->hi)
      throw Panic{CYC_ERR_ARG, n + " must be in " + std::to_string(o->lo) + ".." + std::to_string(o->hi)};
    if (n == "row_phases" && (value == 0 || value > 2)) throw Panic{CYC_ERR_ARG, "row_phases must be -1 (auto), 1 (off) or 2"};
    c->opt.*o->field = n == "pr_group" && value == 0 ? -1 : int(value);
    if (o->stale == Stale::range_plan) c->range.invalidate();  // the next run re-plans
    if (o->stale == Stale::plvt) {  // rebuilt (or not) by the next run
      c->prep.plvt_ready = false;
      c->prep.plvt.alloc(0);
    }
    reroute(c);
    drop_graph(c);
    return (int)CYC_OK;
  });
}

int cyc_get_option(cyc_ctx* c, const char* name, int64_t* value) {
  if (!c || !name || !value) return CYC_ERR_ARG;
  const std::string n(name);
  auto need_prepare = [&] { return fail(c, CYC_ERR_ARG, n + ": call cyc_probe_prepare first"); };
  if (n == "pod_words") {  // the mode in effect, not the option
    if (!c->prepared) return need_prepare();
    *value = c->route.ido ? 1 : 0;
  } else if (const OptionRow* o = find_option(name)) *value = c->opt.*o->field;
  else if (n == "launch") *value = c->route.launch;  // in effect
  else if (n == "front_fused_active") *value = c->route.fused ? 1 : 0;
  else if (n == "pl_wave_active") {
    if (!c->prepared) return need_prepare();
    *value = c->route.pl_wave ? 1 : 0;
  } else if (n == "class_inplace_active") {
    if (!c->prepared || !c->range.valid) return fail(c, CYC_ERR_ARG, "class_inplace_active: run a probe first");
    *value = c->route.inplace ? 1 : 0;
  } else if (n == "emit_interleave_active") {
    if (!c->prepared || !c->range.valid) return fail(c, CYC_ERR_ARG, "emit_interleave_active: run a probe first");
    *value = c->route.emit_interleave ? 1 : 0;
  } else if (n == "plvt_active") *value = c->prep.plvt_ready ? 1 : 0;
  else if (n == "ip_iv_rows") *value = c->range.Rv;  // (the last range plan's interval-built rows)
  else if (n == "ip_range_rows") *value = c->range.Rr;  // (... and its range-built rows)
  else if (n == "pod_post_rows" || n == "pod_scan_rows") {
    // its sparse pod-peer rows, posting-built and scanned: launch C builds them on the fused front of PM builds only
    const bool sparse = c->prepared && c->range.valid && c->route.fused && !c->route.ido && c->route.pod_sparse;
    *value = !sparse ? 0 : n == "pod_post_rows" ? c->range.n_post : c->range.n_scan;
  } else if (n == "row_phases_active") *value = c->run.last.phase_used;  // (the last run's phases; 0: a plain run)
  else if (n == "effects_batches") *value = c->effects.batches;  // (the last cyc_probe_target_effects call)
  else if (n == "effects_launches") *value = c->effects.launches;
  else if (n == "effects_scratch_bytes") *value = int64_t(c->effects.scratch);
  else if (n == "effects_scratch_cap") *value = int64_t(effects_scratch_cap());
  else return fail(c, CYC_ERR_ARG, "unknown option " + n);
  return (int)CYC_OK;
}

// Shared single-cell runner (k_query).  tlist (optional): per (traffic, direction) the matching
// targets in primary-key order, t for an allowing target and -t-1 for a denying one.
static int run_query(cyc_ctx* c, const std::vector<QueryTraffic>& ts, uint8_t* out,
                     std::vector<std::vector<int64_t>>* tlist, bool members_only = false) {
  DeviceGuard dg(c->device);
  std::vector<uint32_t> ext, tdesc;
  Problem q = build_query_problem(c->policy, ts, ext, tdesc);
  DevBuf ls_off, ls_key, ls_val, sel_off, reqs, req_vals, pod_ns, pod_ls, pod_nsls, pod_ip, cidrs, ipbs, ipb_ex, pms, pents,
      peers, descs, dext, dtdesc, tgt0, tgt1, lo0, lo1, hi0, hi1, selres, portok, res, pan, pid;
  upload(ls_off, q.ls_off);
  upload(ls_key, q.ls_key);
  upload(ls_val, q.ls_val);
  upload(sel_off, q.sel_off);
  upload(reqs, q.reqs);
  upload(req_vals, q.req_vals);
  upload(pod_ns, q.pod_ns);
  upload(pod_ls, q.pod_ls);
  upload(pod_nsls, q.pod_nsls);
  upload(pod_ip, q.pod_ip);
  upload(cidrs, q.cidrs);
  upload(ipbs, q.ipbs);
  upload(ipb_ex, q.ipb_ex);
  upload(pms, q.pms);
  upload(pents, q.pents);
  upload(peers, q.peers);
  upload(descs, q.descs);
  upload(dext, ext);
  upload(dtdesc, tdesc);
  upload(tgt0, q.tgt[0]);
  upload(tgt1, q.tgt[1]);
  upload(lo0, q.tns_lo[0]);
  upload(lo1, q.tns_lo[1]);
  upload(hi0, q.tns_hi[0]);
  upload(hi1, q.tns_hi[1]);
  const uint32_t D = uint32_t(std::max<size_t>(q.descs.size(), 1)), M = uint32_t(q.pms.size());
  selres.alloc(std::max<uint64_t>(uint64_t(q.S) * q.L, 16));
  portok.alloc(std::max<uint64_t>(uint64_t(M) * D, 16));
  res.alloc(std::max<size_t>(ts.size(), 16));
  pan.alloc(std::max<size_t>(ts.size() * 4, 16));
  pid.alloc(std::max<size_t>(ts.size() * 4, 16));
  hipStream_t st = nullptr;
  SelArgs sa{};  // (every selector: no sel_list, no dense table)
  sa.S = q.S, sa.L = q.L, sa.nb = grid1(uint64_t(q.S) * q.L, 256);
  sa.sel_off = sel_off.as<uint32_t>(), sa.reqs = reqs.as<DReq>(), sa.req_vals = req_vals.as<uint32_t>();
  sa.ls_off = ls_off.as<uint32_t>(), sa.ls_key = ls_key.as<uint32_t>(), sa.ls_val = ls_val.as<uint32_t>();
  sa.selres = selres.as<uint8_t>();
  launch(k_selectors, sa, st);
  const PortArgs pa{grid1(uint64_t(M) * D, 256), M, D, pms.as<DPortM>(), pents.as<DPortEntry>(), descs.as<DDesc>(), portok.as<uint8_t>()};
  launch(k_portok, pa, st);
  QueryArgs qa{};
  qa.n = uint32_t(ts.size());
  qa.L = q.L;
  qa.D = D;
  qa.pod_ns = pod_ns.as<uint32_t>();
  qa.pod_ls = pod_ls.as<uint32_t>();
  qa.pod_nsls = pod_nsls.as<uint32_t>();
  qa.ext = dext.as<uint32_t>();
  qa.tdesc = dtdesc.as<uint32_t>();
  qa.pod_ip = pod_ip.as<DIP>();
  qa.selres = selres.as<uint8_t>();
  qa.portok = portok.as<uint8_t>();
  qa.tgt[0] = tgt0.as<DTarget>();
  qa.tgt[1] = tgt1.as<DTarget>();
  qa.tns_lo[0] = lo0.as<uint32_t>();
  qa.tns_lo[1] = lo1.as<uint32_t>();
  qa.tns_hi[0] = hi0.as<uint32_t>();
  qa.tns_hi[1] = hi1.as<uint32_t>();
  qa.peers = peers.as<DPeer>();
  qa.ipbs = ipbs.as<DIPBlock>();
  qa.cidrs = cidrs.as<DCidr>();
  qa.ipb_ex = ipb_ex.as<uint32_t>();
  qa.res = res.as<uint8_t>();
  qa.pan = pan.as<uint32_t>();
  qa.pid = pid.as<uint32_t>();
  // per (traffic, direction): one flag per target of the end's namespace
  std::vector<uint64_t> hoff;
  DevBuf doff, dfl;
  uint64_t nfl = 0;
  if (tlist) {
    for (size_t i = 0; i < ts.size(); i++)
      for (int d = 0; d < 2; d++) {
        uint32_t T = uint32_t(d == 0 ? 2 * i + 1 : 2 * i);  // ingress target = dst, egress = src
        uint32_t ns = q.pod_ns[T];
        hoff.push_back(nfl);
        nfl += q.tns_hi[d][ns] - q.tns_lo[d][ns];
      }
    upload(doff, hoff);
    dfl.alloc(std::max<uint64_t>(nfl, 16));
    HIPCHK(hipMemsetAsync(dfl.p, 0, std::max<uint64_t>(nfl, 16), st));
    qa.tflags = dfl.as<uint8_t>();
    qa.toff = doff.as<uint64_t>();
  }
  qa.members_only = members_only ? 1u : 0u;
  k_query<<<grid1(ts.size(), 128), 128, 0, st>>>(qa);
  std::vector<uint8_t> hres(ts.size());
  std::vector<uint32_t> hpan(ts.size()), hpid(ts.size());
  HIPCHK(hipMemcpy(hres.data(), res.p, ts.size(), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(hpan.data(), pan.p, ts.size() * 4, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(hpid.data(), pid.p, ts.size() * 4, hipMemcpyDeviceToHost));
  for (size_t i = 0; i < ts.size(); i++) {
    if (hpan[i]) {  // analyze.go:209-225 prints the earlier traffics, then the reference panics
      if (hpan[i] == QP_SELECTOR) return fail(c, CYC_ERR_PANIC_SELECTOR, "invalid operator");
      if (hpan[i] == QP_IP) return fail(c, CYC_ERR_PANIC_IP, "unable to parse IP '" + q.pod_ip_str[hpid[i]] + "'");
      const std::string& cs = q.cidr_str[hpid[i]];
      return fail(c, CYC_ERR_PANIC_CIDR, "unable to parse CIDR '" + cs + "': invalid CIDR address: " + cs);
    }
    out[i] = hres[i];
  }
  if (tlist) {
    std::vector<uint8_t> hfl(nfl);
    if (nfl) HIPCHK(hipMemcpy(hfl.data(), dfl.p, nfl, hipMemcpyDeviceToHost));
    tlist->assign(ts.size() * 2, {});
    for (size_t i = 0; i < ts.size(); i++)
      for (int d = 0; d < 2; d++) {
        uint32_t T = uint32_t(d == 0 ? 2 * i + 1 : 2 * i);
        uint32_t lo = q.tns_lo[d][q.pod_ns[T]], hi = q.tns_hi[d][q.pod_ns[T]];
        for (uint32_t t = lo; t < hi; t++) {
          uint8_t f = hfl[hoff[2 * i + d] + (t - lo)];
          if (f) (*tlist)[2 * i + d].push_back(f == 1 ? int64_t(t) : -int64_t(t) - 1);
        }
      }
  }
  return (int)CYC_OK;
}

int cyc_query_traffic(cyc_ctx* c, const char* js, size_t len, uint8_t* out, int64_t n) {
  if (!c || !js) return CYC_ERR_ARG;
  if (!c->have_policy) return fail(c, CYC_ERR_ARG, "load a policy first");
  return guarded(c, [&]() -> int {
    auto ts = load_traffics(json::parse(js, len));
    if (int64_t(ts.size()) > n) return fail(c, CYC_ERR_ARG, "output buffer smaller than the traffic list");
    if (ts.empty()) return (int)CYC_OK;
    return run_query(c, ts, out, nullptr);
  });
}

int cyc_query_traffic_tables(cyc_ctx* c, const cyc_traffic_tables* t, uint8_t* out, int64_t n) {
  if (!c || !t) return CYC_ERR_ARG;
  if (!c->have_policy) return fail(c, CYC_ERR_ARG, "load a policy first");
  return guarded(c, [&]() -> int {
    auto ts = load_traffic_tables(*t);
    if (int64_t(ts.size()) > n || (!ts.empty() && !out)) return fail(c, CYC_ERR_ARG, "output buffer smaller than the traffic list");
    if (ts.empty()) return (int)CYC_OK;
    return run_query(c, ts, out, nullptr);
  });
}

static void json_str(std::string& o, const std::string& v) {
  o += '"';
  for (unsigned char ch : v) {
    if (ch == '"' || ch == '\\') {
      o += '\\';
      o += char(ch);
    } else if (ch < 0x20) {
      char b[8];
      snprintf(b, sizeof(b), "\\u%04x", ch);
      o += b;
    } else {
      o += char(ch);
    }
  }
  o += '"';
}

int cyc_query_traffic_targets(cyc_ctx* c, const char* js, size_t len, char* out_json, size_t cap, size_t* needed) {
  if (!c || !js) return CYC_ERR_ARG;
  if (!c->have_policy) return fail(c, CYC_ERR_ARG, "load a policy first");
  return guarded(c, [&]() -> int {
    auto ts = load_traffics(json::parse(js, len));
    std::vector<uint8_t> res(ts.size());
    std::vector<std::vector<int64_t>> tl;
    if (!ts.empty()) {
      int rc = run_query(c, ts, res.data(), &tl);
      if (rc != CYC_OK) return rc;
    }
    std::string o = "[";
    for (size_t i = 0; i < ts.size(); i++) {
      if (i) o += ',';
      o += '{';
      for (int d = 0; d < 2; d++) {
        o += d ? ",\"Egress\":{" : "\"Ingress\":{";
        for (int allow = 1; allow >= 0; allow--) {
          o += allow ? "\"AllowingTargets\":[" : ",\"DenyingTargets\":[";
          bool first = true;
          for (int64_t t : tl[2 * i + d]) {
            if ((t >= 0) != bool(allow)) continue;
            if (!first) o += ',';
            first = false;
            json_str(o, c->policy.dir[d][size_t(t >= 0 ? t : -t - 1)].pk);
          }
          o += ']';
        }
        o += ",\"IsAllowed\":";
        o += (res[i] >> d) & 1 ? "true" : "false";
        o += '}';
      }
      o += ",\"IsAllowed\":";
      o += (res[i] & 3) == 3 ? "true" : "false";
      o += '}';
    }
    o += ']';
    if (needed) *needed = o.size() + 1;
    if (!out_json || cap < o.size() + 1) return fail(c, CYC_ERR_ARG, "output buffer too small (see *needed)");
    memcpy(out_json, o.c_str(), o.size() + 1);
    return (int)CYC_OK;
  });
}

int cyc_query_targets(cyc_ctx* c, const char* js, size_t len, char* out_json, size_t cap, size_t* needed) {
  if (!c || !js) return CYC_ERR_ARG;
  if (!c->have_policy) return fail(c, CYC_ERR_ARG, "load a policy first");
  return guarded(c, [&]() -> int {
    auto ts = load_target_pods(json::parse(js, len));
    std::vector<uint8_t> res(ts.size());
    std::vector<std::vector<int64_t>> tl;
    if (!ts.empty()) {
      int rc = run_query(c, ts, res.data(), &tl, true);
      if (rc != CYC_OK) return rc;
    }
    std::string o = "[";
    for (size_t i = 0; i < ts.size(); i++) {
      o += i ? ",{" : "{";
      for (int d = 0; d < 2; d++) {
        o += d ? "],\"Egress\":[" : "\"Ingress\":[";
        for (size_t x = 0; x < tl[2 * i + d].size(); x++) {
          if (x) o += ',';
          json_str(o, c->policy.dir[d][size_t(tl[2 * i + d][x])].pk);
        }
      }
      o += "]}";
    }
    o += ']';
    if (needed) *needed = o.size() + 1;
    if (!out_json || cap < o.size() + 1) return fail(c, CYC_ERR_ARG, "output buffer too small (see *needed)");
    memcpy(out_json, o.c_str(), o.size() + 1);
    return (int)CYC_OK;
  });
}

}  // extern "C"

// Multi-GPU table assembly: the RCCL communicator and the all-gather of row shards (C ABI included)
#include "comm.hpp"
