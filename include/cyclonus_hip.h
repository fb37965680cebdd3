/* cyclonus_hip.h — C ABI of libcyclonus_hip.so, the MI355X (gfx950) NetworkPolicy verdict engine.
 *
 * Drop-in boundary for the simulated-connectivity path of cyclonus (reference paths are
 * relative to the reference repository, github.com/mattfenwick/cyclonus @ johnSchnake fork):
 *
 *   cyc_policy_build_json   replaces matcher.BuildNetworkPolicies(simplify, netpols)
 *                           pkg/matcher/builder.go:11-26 (+ Policy.Simplify policy.go:176-183)
 *   cyc_policy_load_ir_json accepts json.Marshal(*matcher.Policy) — the already-built Go policy
 *                           a cgo binding holds in SimulatedJobRunner.Policies (jobrunner.go:64-66)
 *   cyc_resources_load_json probe.Resources (pkg/connectivity/probe/resources.go:15-19) as JSON
 *   cyc_probe_prepare       Resources.GetJobsForProbeConfig (resources.go:274-364) for a batch of
 *                           generator.ProbeConfig values (PortProtocol | AllAvailable)
 *   cyc_probe_run           Runner.RunProbeForConfig (jobrunner.go:29-58) -> SimulatedJobRunner.RunJobs
 *                           (jobrunner.go:68-94) -> Policy.IsTrafficAllowed (policy.go:131-174) for
 *                           every (src pod, dst pod, job) cell, as packed bit-planes
 *   cyc_query_traffic       Policy.IsTrafficAllowed for arbitrary matcher.Traffic values, including
 *                           external peers (analyze.go:209-225 query-traffic)
 *
 * Conventions: every function returns a cyc_status; on failure cyc_last_error(ctx) holds the
 * message (for CYC_ERR_PANIC_* it is the text of the Go panic the reference would raise).
 * Inputs are copied during the call (no caller pointer is retained, cgo-safe).  A context is
 * not internally locked: use one per thread.  Plane layout (W = ceil(P/64) 64-bit words):
 *   status[d*K + k]                      cyc_job_status of destination pod d, job slot k
 *   ingress[((d-row_lo)*K + k)*W + s/64]  bit s%64: ingress verdict of s -> d, slot k
 *   egress [((s-row_lo)*K + k)*W + d/64]  bit d%64: egress verdict of s -> d, slot k
 * i.e. each plane is keyed by the pod the direction's policies TARGET (ingress: destination,
 * egress: source; policy.go:143-149).  Combined = ingress AND egress (policy.go:123-125).
 * Bits of non-VALID slots are 0; their Ingress/Egress/Combined follow jobrunner.go:36-55.
 */
#ifndef CYCLONUS_HIP_H
#define CYCLONUS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  CYC_OK = 0,
  CYC_ERR_ARG = 1,             /* bad argument / call order */
  CYC_ERR_JSON = 2,            /* malformed input document */
  CYC_ERR_INVALID_POLICY = 3,  /* builder.go:39,174-181 panics */
  CYC_ERR_PANIC_IP = 4,        /* ippeermatcher.go:46-48 panic: unparsable pod IP */
  CYC_ERR_PANIC_CIDR = 5,      /* ippeermatcher.go:46-48 panic: unparsable CIDR / except */
  CYC_ERR_PANIC_SELECTOR = 6,  /* labelselector.go:57 panic("invalid operator") */
  CYC_ERR_DUPLICATE_KEY = 7,   /* table.go:45 via utils.DoOrDie (log.Fatalf) */
  CYC_ERR_HIP = 8,
  CYC_ERR_OOM = 9,
  CYC_ERR_RCCL = 10,
  CYC_ERR_PANIC_RUNTIME = 11   /* Go runtime panic in the job expansion: a pod without containers is a
                                  job's podFrom (resources.go:296,349, Containers[0]) */
} cyc_status;

typedef enum {
  CYC_JOB_NONE = 0,               /* no job in this slot (AllAvailable, fewer containers) */
  CYC_JOB_VALID = 1,              /* Ingress/Egress from the planes */
  CYC_JOB_BAD_NAMED_PORT = 2,     /* Ingress=invalidnamedport, Egress=unknown (jobrunner.go:47-55) */
  CYC_JOB_BAD_PORT_PROTOCOL = 3   /* Ingress=invalidportprotocol, Egress=unknown (:36-45) */
} cyc_job_status;

typedef struct cyc_ctx cyc_ctx;

typedef struct {
  int64_t pods;        /* P */
  int64_t slots;       /* K: job slots per destination pod over all probe configs */
  int64_t words;       /* W = ceil(P/64) */
  int64_t configs;     /* number of probe configs */
  int64_t targets_in;  /* ingress targets after merge/simplify */
  int64_t targets_eg;
  int64_t peers;
  int64_t classes_in;  /* filled after cyc_probe_run */
  int64_t classes_eg;
  int64_t may_panic;   /* 1 if evaluation can reach a Go panic (invalid CIDR/IP/operator) */
  int64_t selectors;   /* S: distinct label selectors */
  int64_t label_sets;  /* L: distinct pod / namespace label sets */
  int64_t pod_peers;   /* pod-selector peers (pod, namespace or both) */
  int64_t ip_peers;    /* IPBlock peers */
  int64_t descriptors; /* D: distinct job descriptors (port, port name, protocol) */
  int64_t max_word_runs; /* most egress-identity runs in one 64-pod word */
} cyc_probe_shape;

/* ABI revision of this header: bumped whenever a struct's layout or a field's meaning changes.  A
 * binding checks cyc_abi_version() == CYC_ABI_VERSION once at start-up so a library and a binding
 * built against different headers fail loudly instead of misreading each other's structs. */
#define CYC_ABI_VERSION 2

/* context / errors */
int cyc_abi_version(void);
int cyc_ctx_create(int device_id, cyc_ctx** out);
void cyc_ctx_destroy(cyc_ctx* ctx);
const char* cyc_last_error(const cyc_ctx* ctx);
const char* cyc_version(void);

/* policy compile: JSON array (or List / single object) of networking.k8s.io/v1 NetworkPolicy */
int cyc_policy_build_json(cyc_ctx* ctx, int simplify, const char* netpols_json, size_t len);
/* policy load: json.Marshal(*matcher.Policy) produced by the Go reference */
int cyc_policy_load_ir_json(cyc_ctx* ctx, const char* policy_json, size_t len);
/* export the compiled policy as json.Marshal(*matcher.Policy) would; returns bytes needed (+1) and
 * writes the NUL-terminated text when cap holds it (a smaller cap writes nothing); returns
 * -(cyc_status) on failure (no policy loaded, or the dump failed) with cyc_last_error set */
int64_t cyc_policy_ir_json(cyc_ctx* ctx, char* buf, size_t cap);

/* probe model: probe.Resources JSON ({"Namespaces": {...}, "Pods": [...]}) */
int cyc_resources_load_json(cyc_ctx* ctx, const char* resources_json, size_t len);

/* probe configs: JSON array of {"Port": <int|string>, "Protocol": "TCP"} or {"AllAvailable": true};
 * flattens + uploads all tables and allocates device scratch.  Fills *shape. */
int cyc_probe_prepare(cyc_ctx* ctx, const char* probes_json, size_t len, cyc_probe_shape* shape);

/* ---- Flat-table ingestion (no JSON): what a cgo binding passes straight from its Go values.
 * Every string is an index into one string table (duplicates allowed); maps and lists are
 * [n + 1] offset arrays into shared element arrays; optional arrays may be NULL.  The caller keeps
 * ownership: everything is copied during the call (cgo rule: no Go pointer is retained).  Indices
 * and offsets are validated (CYC_ERR_ARG names the first bad one). */
typedef struct {
  int64_t n;           /* strings */
  const char* bytes;   /* their bytes, concatenated (Go strings: any bytes, NUL included) */
  const int64_t* off;  /* [n + 1]: string i = bytes[off[i], off[i + 1]) */
} cyc_strings;

/* probe.Resources (pkg/connectivity/probe/resources.go:15-19, pod.go:44-51,173-179) */
typedef struct {
  cyc_strings str;
  /* Namespaces map[string]map[string]string */
  int64_t n_namespaces;
  const int32_t* ns_name;        /* [n_namespaces] the map key */
  const uint8_t* ns_nil;         /* [n_namespaces] 1: a nil label map (optional) */
  const int64_t* ns_label_off;   /* [n_namespaces + 1] into ns_label_key / ns_label_val */
  const int32_t *ns_label_key, *ns_label_val;
  /* Pods []*Pod, in order */
  int64_t n_pods;
  const int32_t *pod_ns, *pod_name, *pod_ip;  /* [n_pods] Namespace, Name, IP */
  const int64_t* pod_label_off;  /* [n_pods + 1] into label_key / label_val (Labels map) */
  const int32_t *label_key, *label_val;
  const int64_t* pod_cont_off;   /* [n_pods + 1] into the container arrays (Containers) */
  const int32_t *cont_name, *cont_port, *cont_proto, *cont_port_name;  /* Name, Port, Protocol, PortName */
  const uint8_t* pod_nil;        /* [n_pods] optional: bit 0 Labels == nil, bit 1 Containers == nil
                                    (json.Marshal fidelity only: cyc_resources_json writes null) */
} cyc_resource_tables;

/* generator.ProbeConfig (pkg/generator/probeconfig.go): AllAvailable, or PortProtocol{Port intstr, Protocol} */
typedef struct {
  int32_t all_available;  /* 1: one job per destination container (resources.go:336-364) */
  int32_t port_is_name;   /* intstr.Type: 0 Int (port), 1 String (port_name) */
  int32_t port;
  /* Go strings as (pointer, byte length): any bytes, NUL included; NULL with length 0 = "".
   * (ABI 2 renamed the pointers from port_name / protocol when the lengths were added, so a caller
   * written against ABI 1 that set only the pointer no longer compiles.) */
  const char* port_name_ptr;  /* the named port */
  int64_t port_name_len;
  const char* protocol_ptr;   /* the raw protocol string (compared as is: "tcp" != "TCP") */
  int64_t protocol_len;
} cyc_probe_config;

/* *matcher.Policy after BuildNetworkPolicies (+ Simplify) (pkg/matcher/policy.go:11-14,
 * target.go:11-23, peermatcher.go, podpeermatcher.go, ippeermatcher.go, portmatcher.go): the already
 * built Go policy, flattened.  Targets are given per direction (ingress then egress); each holds its
 * ordered peer list; a peer's port matcher is an index (peers of one rule may share one). */
typedef enum { CYC_PEER_ALL = 0, CYC_PEER_PORTS = 1, CYC_PEER_POD = 2, CYC_PEER_IP = 3 } cyc_peer_kind;
typedef enum { CYC_NS_EXACT = 0, CYC_NS_ALL = 1, CYC_NS_LABEL = 2 } cyc_ns_kind;
typedef enum { CYC_PORT_ANY = 0, CYC_PORT_NUMBER = 1, CYC_PORT_NAME = 2 } cyc_port_kind;
typedef struct {
  cyc_strings str;
  /* metav1.LabelSelector: MatchLabels, then MatchExpressions {Key, Operator, Values} */
  int64_t n_selectors;
  const int64_t* sel_label_off;  /* [n_selectors + 1] into sel_label_key / sel_label_val */
  const int32_t *sel_label_key, *sel_label_val;
  const int64_t* sel_expr_off;   /* [n_selectors + 1] into expr_key / expr_op / expr_value_off */
  const int32_t *expr_key, *expr_op;  /* expr_op: the operator text ("In", "NotIn", "Exists", "DoesNotExist";
                                         anything else panics when reached, labelselector.go:57) */
  const int64_t* expr_value_off; /* [n_exprs + 1] into expr_value */
  const int32_t* expr_value;
  /* PortMatcher: AllPortMatcher, or SpecificPortMatcher{Ports, PortRanges} */
  int64_t n_port_matchers;
  const uint8_t* pm_all;         /* [n_port_matchers] 1: AllPortMatcher */
  const uint8_t *pm_ports_nil, *pm_ranges_nil;  /* optional: nil slices (json.Marshal fidelity only) */
  const int64_t* pm_port_off;    /* [n_port_matchers + 1] into port_* (PortProtocolMatcher) */
  const uint8_t* port_kind;      /* cyc_port_kind: Port == nil / number / name */
  const int32_t* port_value;     /* the number, or the name's string index */
  const int32_t* port_proto;     /* Protocol string index */
  const int64_t* pm_range_off;   /* [n_port_matchers + 1] into range_* (PortRangeMatcher) */
  const int32_t *range_from, *range_to, *range_proto;
  /* targets: n_targets[0] ingress, then n_targets[1] egress, each direction sorted or not (the
   * library orders them by primary key, target.go:57-62, as Go's map keys) */
  int64_t n_targets[2];
  const int32_t* target_ns;      /* Namespace string index */
  const int32_t* target_sel;     /* PodSelector: selector index */
  const uint8_t* target_peers_nil; /* optional: Peers == nil (json.Marshal fidelity only) */
  const int64_t* target_peer_off;  /* [n_in + n_eg + 1] into peer_* (ordered: Target.Allows short-circuits) */
  const int64_t* target_rule_off;  /* optional [n_in + n_eg + 1] into rule_name (SourceRules' names) */
  const int32_t* rule_name;
  /* peers */
  const uint8_t* peer_kind;      /* cyc_peer_kind */
  const int32_t* peer_port;      /* port matcher index (ignored for CYC_PEER_ALL) */
  const uint8_t* peer_ns_kind;   /* cyc_ns_kind (pod peers) */
  const int32_t* peer_ns;        /* CYC_NS_EXACT: namespace string index; CYC_NS_LABEL: selector index */
  const int32_t* peer_pod_sel;   /* pod peers: selector index, -1 = all pods */
  const int32_t* peer_cidr;      /* IP peers: CIDR string index */
  const int64_t* peer_except_off;  /* [n_peers + 1] into except_cidr (IP peers' Except) */
  const uint8_t* peer_except_nil;  /* optional: Except == nil (json.Marshal fidelity only) */
  const int32_t* except_cidr;
} cyc_policy_tables;

/* the flat counterparts of cyc_resources_load_json, cyc_policy_load_ir_json and cyc_probe_prepare */
int cyc_resources_load(cyc_ctx* ctx, const cyc_resource_tables* tables);
int cyc_policy_load(cyc_ctx* ctx, const cyc_policy_tables* tables);
int cyc_probe_prepare_configs(cyc_ctx* ctx, const cyc_probe_config* configs, int64_t n, cyc_probe_shape* shape);
/* the loaded probe model as json.Marshal(*probe.Resources) would write it (Pod.ServiceIP and
 * Container.BatchJobs are not kept; nil label maps and container slices as null: from JSON input an
 * absent or null field, from flat tables ns_nil / pod_nil); returns bytes needed (+1) or
 * -(cyc_status), as cyc_policy_ir_json */
int64_t cyc_resources_json(cyc_ctx* ctx, char* buf, size_t cap);

/* Compute the verdict planes on the GPU for target-pod rows [row_lo, row_hi) (rows are pods in
 * Resources.Pods order; pass 0, P for the whole table).  Device pointers; `hip_stream` is the
 * hipStream_t to enqueue on (NULL = the HIP default stream, as with every HIP API).  Asynchronous
 * unless the inputs can panic (then it synchronises to report the first panicking job in job
 * order, as the reference would).  The planes must be device memory (hipMalloc and the like), read
 * back by hipMemcpy or by kernels after the stream: the run's events release at device scope, so
 * host-mapped, non-coherent memory is not made visible to the host by a stream synchronisation.
 * Alignment: d_ingress and d_egress are planes of 64-bit words and must be 8-byte aligned; a pointer
 * that is not is refused with CYC_ERR_ARG (the message names the argument) before anything is
 * enqueued, here and in cyc_probe_run_rows, cyc_table_wrap and cyc_table_wrap_rows.  16-byte aligned
 * planes (hipMalloc's are) enable the vector paths: the 16-byte emit kernels (when the plane rows are
 * an even number of words too) and the class rows' 16-byte pair stores; 8-byte aligned planes get the
 * same bits through 8-byte stores (cyc_last_emit then names k_emit_words).  d_status has no
 * alignment requirement.  The library writes exactly the planes' bytes, nothing before or after. */
int cyc_probe_run(cyc_ctx* ctx, void* hip_stream, uint64_t* d_ingress, uint64_t* d_egress, uint8_t* d_status,
                  int64_t row_lo, int64_t row_hi);

/* Same, into host buffers (allocates + copies; synchronous). */
int cyc_probe_run_host(cyc_ctx* ctx, uint64_t* ingress, uint64_t* egress, uint8_t* status, int64_t row_lo,
                       int64_t row_hi);

/* ---- Row partitions for one-process-per-GPU runs (north_star: "source-pod rows shard across the
 * GPUs").  A rank runs rows [row_lo, row_hi) of the pods under one of two partitions:
 *   CYC_ROWS_TARGET  the rows are TARGET pods of both planes (cyc_probe_run's layout above): rank r
 *                    holds the ingress rows of destinations and the egress rows of sources in the range.
 *   CYC_ROWS_SOURCE  the rows are SOURCE pods: rank r holds every cell (s in [row_lo, row_hi), d, k),
 *                    i.e. Table.Get(from, *) for its sources (pkg/connectivity/probe/table.go:54-56, the
 *                    reference's jobs are generated source-major, resources.go:286-287):
 *                      egress [((s - row_lo)*K + k)*W  + d/64]              bit d%64 (full rows of its sources)
 *                      ingress[(d*K + k)*Wr + (s/64 - row_lo/64)]          bit s%64, for EVERY destination d,
 *                    Wr = ceil(row_hi/64) - row_lo/64 words: the rank's slice of each ingress row.
 *                    row_lo must be a multiple of 64, and row_hi too unless it is P, so the slices of
 *                    a partition tile every ingress row.  The rank's peer rows and ingress class rows
 *                    cover only its words, so its front work shrinks with the partition too.
 * The union of the ranks' planes is the whole table either way, with no data exchange (the inputs are
 * replicated); assembling it on every rank is one all-gather per plane (cyclonus_amd/shard.py). */
typedef enum { CYC_ROWS_TARGET = 0, CYC_ROWS_SOURCE = 1 } cyc_rows;

/* Plane shapes of rows [row_lo, row_hi) under `partition`: out[0] ingress rows, out[1] words per
 * ingress (row, slot), out[2] egress rows, out[3] words per egress (row, slot), out[4] the ingress
 * window's first word (0 for target rows).  Needs cyc_probe_prepare. */
int cyc_rows_layout(cyc_ctx* ctx, int partition, int64_t row_lo, int64_t row_hi, int64_t* out, int n);
/* cyc_probe_run under a partition.  Plane alignment: as cyc_probe_run (8-byte aligned planes, or CYC_ERR_ARG). */
int cyc_probe_run_rows(cyc_ctx* ctx, void* hip_stream, uint64_t* d_ingress, uint64_t* d_egress, uint8_t* d_status,
                       int partition, int64_t row_lo, int64_t row_hi);
int cyc_probe_run_host_rows(cyc_ctx* ctx, uint64_t* ingress, uint64_t* egress, uint8_t* status, int partition,
                            int64_t row_lo, int64_t row_hi);

/* ---- Which target decides: per-target effect counts over the verdict grid.
 * For every cell the reference's Policy.IsIngressOrEgressAllowed (pkg/matcher/policy.go:138-174) sorts each
 * target that applies to the cell's target pod into DirectionResult.AllowingTargets or .DenyingTargets
 * (policy.go:84-96), and SimulatedJobRunner.RunJob renders that result per job (jobrunner.go:80).  The
 * planes keep only the final bit; this call counts, per target t and job slot k, the cells of each kind
 * without visiting them (bit rows of 64 pods).
 *   direction  CYC_DIR_INGRESS counts over Policy.Ingress, CYC_DIR_EGRESS over Policy.Egress.  T below is
 *              cyc_probe_shape.targets_in / targets_eg, and target index t is the primary-key order that
 *              cyc_policy_ir_json and cyc_query_traffic_targets use.
 *   rows       [row_lo, row_hi) are the pods the direction's policies TARGET: destinations for ingress,
 *              sources for egress — cyc_probe_run's target rows, so the outputs of the shards of a row
 *              partition add up to the whole table's.  The other end of a cell ranges over all P pods, a
 *              pod's cell with itself included.
 *   jobs       only VALID jobs count (status[d][k] == CYC_JOB_VALID, d the cell's destination): the
 *              reference evaluates no policy for the other job kinds (jobrunner.go:36-55).
 *   effects    host array, exactly T * nk * 4 elements written (nk = k_hi - k_lo); element
 *              [(t*nk + k-k_lo)*4 + e] is the number of cells (s, d, k) of the range with
 *                CYC_EFFECT_ALLOWING       t in AllowingTargets
 *                CYC_EFFECT_DENYING        t in DenyingTargets
 *                CYC_EFFECT_SOLE_ALLOWING  AllowingTargets == [t] and DenyingTargets is not empty: another
 *                                          target applies and denies, so without t this direction's verdict
 *                                          turns from allowed to blocked
 *                CYC_EFFECT_SOLE_DENYING   DenyingTargets == [t] and AllowingTargets is empty: t is the only
 *                                          target that applies, so without it the verdict turns to allowed
 *                                          (policy.go:158-160)
 *              SOLE_ALLOWING + SOLE_DENYING of t is therefore exactly the number of direction verdicts that
 *              depend on t alone; a target with both zero over all slots can be removed without changing
 *              any verdict of this probe.
 *   applies    optional host array [T]: the pods of the rows t applies to (TargetsApplyingToPod,
 *              policy.go:68-82).
 * Needs cyc_probe_prepare or cyc_probe_prepare_configs and no run; synchronous; may be called at any time
 * between runs.  It reads only what a prepare made and works in scratch it allocates and frees: the range
 * plan, a captured graph, cyc_last_* and the options are as they were.  CYC_ERR_ARG (cyc_last_error names
 * the problem): no prepare, a batched-blocks prepare, an unknown direction, a row or slot range out of
 * bounds, NULL effects, and a problem with cyc_probe_shape.may_panic — take the panic from cyc_probe_run;
 * the reference would die at its first such job.  An empty slot range, T == 0 and row_lo == row_hi are not
 * errors: the (possibly zero) elements are written as zeros. */
typedef enum { CYC_DIR_INGRESS = 0, CYC_DIR_EGRESS = 1 } cyc_direction;
enum { CYC_EFFECT_ALLOWING = 0, CYC_EFFECT_DENYING = 1, CYC_EFFECT_SOLE_ALLOWING = 2, CYC_EFFECT_SOLE_DENYING = 3 };
int cyc_probe_target_effects(cyc_ctx* ctx, int direction, int64_t row_lo, int64_t row_hi, int64_t k_lo, int64_t k_hi,
                             int64_t* effects, int64_t* applies);

/* ---- Device-resident verdict tables: the lazy probe.Table (pkg/connectivity/probe/table.go:24-56).
 * The reference's Runner.RunProbeForConfig returns *Table = NewTableFromJobResults(resources,
 * runProbe(jobs)) (jobrunner.go:29-58, table.go:38-48): one Item per (from, to) pod pair holding a
 * JobResult {Ingress, Egress, Combined} per job key.  A cyc_table keeps the packed planes on the GPU
 * and hands out those Connectivity values for any block of cells, so a binding never builds the
 * P^2*K Job structs of resources.go:284-364. */
typedef enum { /* probe.Connectivity, in the order of AllConnectivity (connectivity.go:16-23) */
  CYC_CONN_UNKNOWN = 0,
  CYC_CONN_CHECK_FAILED = 1,
  CYC_CONN_INVALID_NAMED_PORT = 2,
  CYC_CONN_INVALID_PORT_PROTOCOL = 3,
  CYC_CONN_BLOCKED = 4,
  CYC_CONN_ALLOWED = 5,
  CYC_CONN_NO_JOB = 255 /* no job in this slot: the Item has no JobResult for it */
} cyc_connectivity;

typedef struct cyc_table cyc_table;

/* Run the probe for target rows [row_lo, row_hi) into planes the table owns (synchronous; panics
 * are reported as by cyc_probe_run).  A table stays valid after its context is destroyed. */
int cyc_table_run(cyc_ctx* ctx, int64_t row_lo, int64_t row_hi, cyc_table** out);
/* A table over planes the caller produced with cyc_probe_run (device pointers, not owned; they
 * must outlive the table and the run must be complete before cyc_table_cells).  Plane alignment: as
 * cyc_probe_run (8-byte aligned planes, or CYC_ERR_ARG). */
int cyc_table_wrap(cyc_ctx* ctx, const uint64_t* d_ingress, const uint64_t* d_egress, const uint8_t* d_status,
                   int64_t row_lo, int64_t row_hi, cyc_table** out);
/* The same under a row partition (cyc_probe_run_rows; cyc_table_wrap_rows: plane alignment as
 * cyc_probe_run).  A CYC_ROWS_SOURCE table answers every cell
 * (s, d, k) with s inside its rows: Ingress, Egress and Combined of Table.Get(from = s, to = d). */
int cyc_table_run_rows(cyc_ctx* ctx, int partition, int64_t row_lo, int64_t row_hi, cyc_table** out);
int cyc_table_wrap_rows(cyc_ctx* ctx, const uint64_t* d_ingress, const uint64_t* d_egress, const uint8_t* d_status,
                        int partition, int64_t row_lo, int64_t row_hi, cyc_table** out);
/* Connectivity of every cell (s, d, k) of sources [s_lo,s_hi) x destinations [d_lo,d_hi) x slots
 * [k_lo,k_hi), computed on the device, into host arrays indexed
 *   ((s - s_lo) * (d_hi - d_lo) + (d - d_lo)) * (k_hi - k_lo) + (k - k_lo)
 * ingress / egress / combined are each optional (NULL = not wanted): JobResult.Ingress, .Egress and
 * .Combined of that job (jobrunner.go:36-55,85-93).  Target rows: ingress needs the destinations
 * inside the table's rows, egress the sources, combined both.  Source rows: every output needs the
 * sources inside the table's rows (any destination). */
int cyc_table_cells(cyc_table* t, int64_t s_lo, int64_t s_hi, int64_t d_lo, int64_t d_hi, int64_t k_lo, int64_t k_hi,
                    uint8_t* ingress, uint8_t* egress, uint8_t* combined);
/* ---- Whole-table consumers, computed where the planes are (synchronous, on the table's own stream
 * like cyc_table_cells; valid after the context is destroyed).  Both make one pass over the planes of
 * the slot range (no host copy of a plane); plane bits at or beyond P and bits of non-VALID slots are
 * ignored (a wrapped plane is the caller's memory).  Accepted tables: a whole target-row table (row_lo = 0, row_hi = P) or a
 * CYC_ROWS_SOURCE table, which answers the cells (s in its rows, every d, k), so the results of a
 * partition's shards add up to the whole table's.  Failures: CYC_ERR_ARG with cyc_table_error(t)
 * (of `a` for cyc_table_compare).
 *
 * Connectivity counts of slots [k_lo, k_hi) over every cell the table answers: the Result / Printer
 * summaries.  out arrays (host, each optional, at least one): [(k - k_lo) * 6 + c] = number of cells
 * (s, d, k) whose JobResult.Ingress / .Egress / .Combined is cyc_connectivity c (0..5), mapping as
 * cyc_table_cells (jobrunner.go:36-55,85-93); *no_job (optional) = cells with CYC_CONN_NO_JOB.
 * A partial target-row table is accepted when combined and no_job are NULL: Ingress is counted over
 * its destinations (every source), Egress over its sources (every destination). */
int cyc_table_counts(cyc_table* t, int64_t k_lo, int64_t k_hi, int64_t* ingress, int64_t* egress, int64_t* combined,
                     int64_t* no_job);
/* connectivity.NewComparisonTableFrom(a, b) (pkg/connectivity/comparisontable.go:46-67) without
 * building the Items: Combined of a (the kube probe) against Combined of b (the simulated one), slots
 * [k_lo, k_hi), a cell's Combined code being cyc_table_cells' (CYC_CONN_NO_JOB included).
 *   pair_counts[3]  ValueCounts (:109-123): (from, to) pairs that are same, different, ignored.  A pair
 *                   is same iff the codes agree in every slot of the range, NO_JOB included
 *                   (Item.IsSuccess = equalsDict :22-36: a job's key depends on (to, slot) only, so equal
 *                   key sets are equal NO_JOB patterns); ignored iff ignore_loopback and from == to.
 *   slot_counts     optional host [(k - k_lo) * 3 + {same, different, ignored}]: per job, every cell
 *                   where a holds a job counted once: ignored when ignore_loopback and s == d (the
 *                   loopback test comes before success, ValueCountsByProtocol :89-107), else same iff
 *                   b's code equals a's (Item.ResultsByProtocol :14-20); a job b lacks is different (the
 *                   reference would dereference nil there).
 *   dst_counts      optional host [(d * (k_hi - k_lo) + k - k_lo) * 3 + ...]: the same per destination.
 *   d_diff          optional DEVICE plane [P][W] ([P][Wr] over a source table's ingress window), 8-byte
 *                   aligned (or CYC_ERR_ARG): RenderSuccessTable's matrix (:125-134) keyed by destination
 *                   like the ingress plane, row d bit s set iff the Items (s, d) differ; loopback is not
 *                   special; bits at or beyond P are 0; exactly the plane's bytes are written.
 * a and b must be on one device with equal P, K, partition and rows; the status planes may differ. */
int cyc_table_compare(cyc_table* a, cyc_table* b, int64_t k_lo, int64_t k_hi, int ignore_loopback, int64_t pair_counts[3],
                      int64_t* slot_counts, int64_t* dst_counts, uint64_t* d_diff);
/* ---- Which cells: the listing behind a count (the reference walks Wrapped.Keys() and prints whole
 * tables, printer.go:243-263, comparisontable.go:62-64,125-134; here the answer is a list of the matching
 * cells).  Accepted tables, stream, lifetime, plane bits at or beyond P and failures: as for
 * cyc_table_counts / cyc_table_compare above (a partial target-row table is refused). */
typedef enum { CYC_VIEW_INGRESS = 0, CYC_VIEW_EGRESS = 1, CYC_VIEW_COMBINED = 2 } cyc_view;
typedef struct {            /* 16 bytes */
  uint32_t s, d, k;         /* from pod, to pod, slot (plane order) */
  uint8_t ingress, egress, combined;  /* JobResult of the table (of `a`), cyc_table_cells' codes */
  uint8_t other;            /* compare: b's Combined code (CYC_CONN_NO_JOB possible); find: 0 */
} cyc_cell;
/* The cells (s, d, k), k in [k_lo, k_hi), whose code in `view` (cyc_view) is a cyc_connectivity c in 0..5
 * with bit c of code_mask set (0, or bits >= 6: CYC_ERR_ARG).  A CYC_CONN_NO_JOB cell is not a job and
 * never matches; a status-only code (the two invalid kinds, Egress unknown) matches for every source of
 * that (d, k).
 * Order and paging: `cells` (host memory, room for `cap` records) receives ALL matching cells of sources
 * [s_from, *s_next) in ascending (s, d, k) order, *n of them; records at index >= *n are not touched.
 * *s_next is the largest source <= row_hi for which they fit into cap (it runs over trailing sources
 * without matches and is row_hi when everything fits); *total = matching cells of sources
 * [s_from, row_hi).  Continue with s_from = *s_next until it equals row_hi.  cap >= P * (k_hi - k_lo)
 * always makes progress; if source s_from alone has more matches than cap the call is CYC_ERR_ARG (the
 * message names the source and its count; *total is still set).  cells == NULL with cap == 0 is a
 * count-only call: *n = 0, *s_next = s_from, never an error of that kind.  s_from == row_hi: *n = 0,
 * *total = 0; an empty slot range: *n = 0, *s_next = row_hi, *total = 0.  s_from outside [row_lo, row_hi],
 * a bad slot range, a negative cap, NULL cells with cap > 0, NULL n, s_next or total: CYC_ERR_ARG.  The
 * records are the same from run to run. */
int cyc_table_find(cyc_table* t, int view, uint32_t code_mask, int64_t k_lo, int64_t k_hi, int64_t s_from,
                   cyc_cell* cells, int64_t cap, int64_t* n, int64_t* s_next, int64_t* total);
/* The same listing of exactly the cells cyc_table_compare counts as `different` in slot_counts: a holds
 * a job there, b's Combined code differs from a's (or b lacks the job), and the cell is not an ignored
 * loopback.  a and b must match as in cyc_table_compare. */
int cyc_table_compare_find(cyc_table* a, cyc_table* b, int64_t k_lo, int64_t k_hi, int ignore_loopback,
                           int64_t s_from, cyc_cell* cells, int64_t cap, int64_t* n, int64_t* s_next, int64_t* total);
/* ---- The middle level between the totals and the listings: counts and comparison per pair of pod groups
 * (which namespaces reach which; between which the two tables disagree).  The reference has no such summary:
 * it prints whole pod tables (table.go:58-156, comparisontable.go:125-134).  The grouping is the caller's:
 * group_of is a host int32[P], copied during the call; group_of[p] in [0, n_groups) or -1 = pod p is left out
 * as source and as destination.  Any other value: CYC_ERR_ARG naming the first bad index.  n_groups >= 1 and
 * n_groups^2 * max(k_hi - k_lo, 1) <= 2^27 (else CYC_ERR_ARG naming the limit).  Accepted tables as for
 * cyc_table_find (a whole target-row table or a CYC_ROWS_SOURCE table; the shards of a partition add up to the
 * whole table's result; a partial target-row table is refused); stream, lifetime, failures, plane bits at or
 * beyond P and plane alignment as for cyc_table_counts: one pass over the planes, G = n_groups and
 * nk = k_hi - k_lo below.  NULL group_of, a bad slot range or no output: CYC_ERR_ARG.  Exactly the stated
 * number of elements of each output array is written; an empty slot range or P = 0 writes zeros (group_counts)
 * and returns CYC_OK.
 *
 * ingress / egress / combined (host, each optional; at least one output, no_job included):
 *   [((gs * G + gd) * nk + (k - k_lo)) * 6 + c] = number of cells (s, d, k) with group_of[s] == gs,
 *   group_of[d] == gd and cyc_connectivity code c in that view: the codes of cyc_table_cells and
 *   cyc_table_counts (a status-only code counts once for every source of the destination).
 * no_job (optional): [gs * G + gd] = the cells with CYC_CONN_NO_JOB.
 * When no pod is -1 the sums over (gs, gd) are cyc_table_counts' results. */
int cyc_table_group_counts(cyc_table* t, const int32_t* group_of, int64_t n_groups, int64_t k_lo, int64_t k_hi,
                           int64_t* ingress, int64_t* egress, int64_t* combined, int64_t* no_job);
/* cyc_table_compare split by group pair (a and b must match as there):
 *   pair_counts  [(gs * G + gd) * 3 + {same, different, ignored}]: (from, to) pairs; a pair is ignored iff
 *                ignore_loopback and from == to, so ignored pairs land in (g, g).  Required.
 *   slot_counts  optional [((gs * G + gd) * nk + k - k_lo) * 3 + ...]: per job as cyc_table_compare's slot_counts
 *                (only cells where a holds a job, loopback tested before success, a job b lacks is different).
 * When no pod is -1 the sums over (gs, gd) are cyc_table_compare's pair_counts and slot_counts. */
int cyc_table_group_compare(cyc_table* a, cyc_table* b, const int32_t* group_of, int64_t n_groups, int64_t k_lo,
                            int64_t k_hi, int ignore_loopback, int64_t* pair_counts, int64_t* slot_counts);
/* ---- The pod level: counts and comparison per source pod and per destination pod (which pods reach everything
 * or nothing; on which pods the differences of two tables sit: an egress-side fault shows per source, an
 * ingress-side one per destination).  The reference has no such summary.  Accepted tables as for cyc_table_find
 * (a partial target-row table is refused); stream, lifetime, failures, plane bits at or beyond P and plane
 * alignment as for cyc_table_counts: one pass over the planes.  Below rows = row_hi - row_lo, nk = k_hi - k_lo,
 * r = s - row_lo.  Exactly the stated number of elements of each output array is written.
 *
 * view: a cyc_view.  Column c of a row of 7: c in 0..5 the cells with cyc_connectivity code c in that view (the
 * codes of cyc_table_cells), [6] the cells without a job (CYC_CONN_NO_JOB).  Outputs (host, each optional, at
 * least one):
 *   by_src  [(r * nk + k - k_lo) * 7 + c]: for source s of the table's rows, the destinations d in [0, P) whose
 *           cell (s, d, k) has that code; every (r, k) row sums to P.
 *   by_dst  [(d * nk + k - k_lo) * 7 + c]: for every destination d in [0, P), the sources of the table's rows;
 *           every (d, k) row sums to rows.
 * Summed over the pods, the columns 0..5 of either array are cyc_table_counts' result for that view and the sum
 * of column 6 is its no_job.  The by_dst of a source partition's shards add up to the whole table's; their by_src
 * are its rows [row_lo, row_hi).  A bad view or slot range, both outputs NULL: CYC_ERR_ARG.  An empty slot range
 * writes nothing; rows == 0 writes by_dst's zeros. */
#define CYC_POD_CODES 7 /* cyc_connectivity 0..5, then [6] = cells without a job (CYC_CONN_NO_JOB) */
int cyc_table_pod_counts(cyc_table* t, int view /* cyc_view */, int64_t k_lo, int64_t k_hi, int64_t* by_src,
                         int64_t* by_dst);
/* cyc_table_compare per pod (a and b must match as there; no d_diff).  Each output (host, optional, at least
 * one) is {same, different, ignored} under cyc_table_compare's rules:
 *   src_pairs  [r * 3 + x]: the pairs (from = s, to = d) over every d; ignored iff ignore_loopback and s == d.
 *   dst_pairs  [d * 3 + x]: the pairs over the sources of the table's rows (an ignored pair only when d is one).
 *   src_slots  [(r * nk + k - k_lo) * 3 + x]: per job as slot_counts (only cells where a holds a job, loopback
 *              tested before success, a job b lacks is different), over every d.
 *   dst_slots  [(d * nk + k - k_lo) * 3 + x]: element for element cyc_table_compare's dst_counts.
 * Summed over the pods, src_pairs and dst_pairs are cyc_table_compare's pair_counts, src_slots and dst_slots its
 * slot_counts. */
int cyc_table_pod_compare(cyc_table* a, cyc_table* b, int64_t k_lo, int64_t k_hi, int ignore_loopback,
                          int64_t* src_pairs, int64_t* dst_pairs, int64_t* src_slots, int64_t* dst_slots);
/* ---- Multi-hop reachability: what a pod gets to through other pods and in how many hops; which pods get to it.
 * The reference has no such summary.  There is an edge s -> d iff some slot k in [k_lo, k_hi) has
 * status[d][k] == CYC_JOB_VALID, the ingress bit (d, k, s) and the egress bit (s, k, d) set: a Combined of
 * CYC_CONN_ALLOWED (policy.go:123-125) with the codes of cyc_table_cells.  Plane bits at or beyond P and bits of
 * non-VALID slots never make an edge; a loopback edge s -> s is kept in the adjacency plane and cannot change a reach
 * result.  Accepted tables: one that answers every cell, i.e. a whole target-row table or a CYC_ROWS_SOURCE table
 * over rows [0, P); any other table is refused with the text of a partial target-row table (reach over the shards
 * of a partition is not offered).  Stream, lifetime, failures and plane alignment as for cyc_table_counts; neither
 * call changes the table, the context, its options or cyc_last_*.  An unknown direction or a bad slot range:
 * CYC_ERR_ARG.
 *
 * cyc_table_adjacency: one pass over the planes of the slot range into d_adj, a DEVICE plane [P][W], 8-byte aligned
 * (or CYC_ERR_ARG naming d_adj), synchronous on the table's stream like cyc_table_compare's d_diff:
 *   CYC_REACH_FROM  row s, bit d set iff there is an edge s -> d
 *   CYC_REACH_TO    row d, bit s set iff there is an edge s -> d (the transpose)
 * Bits at or beyond P are 0; exactly the plane's bytes are written; an empty slot range writes zeros. */
typedef enum { CYC_REACH_FROM = 0, CYC_REACH_TO = 1 } cyc_reach_direction;
int cyc_table_adjacency(cyc_table* t, int64_t k_lo, int64_t k_hi, int direction /* cyc_reach_direction */, uint64_t* d_adj);
/* Breadth-first search over those edges for n_sets seed sets at once.  Seed set j is
 * seeds[seed_off[j] .. seed_off[j + 1]): pod indices, duplicates allowed, a set may be empty; seed_off has
 * n_sets + 1 entries.  All arrays are host arrays, copied during the call.  max_hops >= 0 bounds the path length,
 * max_hops < 0 runs to the fixpoint.  Outputs (host, each optional, at least one):
 *   hops    [j * P + p]: CYC_REACH_FROM the least h >= 0 such that a path of h edges leads from some seed of set j
 *           to p, CYC_REACH_TO from p to some seed of set j; seeds are 0; -1 when no path of at most max_hops
 *           edges exists.
 *   reach   [j * W + p / 64] bit p % 64 set iff hops >= 0; bits at or beyond P are 0.
 *   levels  [j]: the largest hop value of set j, -1 for an empty set.
 * Exactly the stated number of elements of each output is written, and only when the call succeeds; n_sets == 0
 * writes nothing and returns CYC_OK.  The results are exact and the same from run to run.  The adjacency plane
 * (P rows of W words rounded up to 16), three bitsets of n_sets * W words and, with hops, n_sets * P 32-bit values
 * are device scratch of the call, freed before it returns; an allocation that fails is CYC_ERR_OOM with a message.
 * Limit: n_sets * max(W, 1) <= 2^24 words (else CYC_ERR_ARG stating the limit).  Also CYC_ERR_ARG, each with its
 * message: negative n_sets; NULL seed_off; a seed_off that does not start at 0 or decreases; NULL seeds when a set
 * has a seed; a seed outside [0, P) (the message names the first bad index and its value); all outputs NULL. */
int cyc_table_reach(cyc_table* t, int64_t k_lo, int64_t k_hi, int direction /* cyc_reach_direction */,
                    const int64_t* seed_off, const int32_t* seeds, int64_t n_sets, int64_t max_hops, uint64_t* reach,
                    int32_t* hops, int64_t* levels);
/* ---- All pairs at once: the reflexive transitive closure of those edges, and the zones read off it (how far each
 * pod gets, from how many pods it is reached, which pods all reach one another).  The reference has no such summary.
 * Edges, accepted tables and their refusal text, stream, lifetime, failures and plane alignment as for
 * cyc_table_reach; neither call changes the table, the context, its options or cyc_last_*.  Outputs are written only
 * when the call succeeds; the results are exact and the same from run to run.  An unknown direction or a bad slot
 * range: CYC_ERR_ARG.
 *
 * cyc_table_closure: row p of the closure is the `reach` row cyc_table_reach returns for the seed set {p} with the same
 * slot range and direction and max_hops < 0:
 *   CYC_REACH_FROM  row p, bit q set iff a path of >= 0 edges leads from p to q
 *   CYC_REACH_TO    row p, bit q set iff such a path leads from q to p (the transpose)
 * Bit p of row p is always set, a loopback edge changes nothing, bits at or beyond P are 0; an empty slot range gives
 * the identity.  Outputs (each optional, at least one, or CYC_ERR_ARG):
 *   d_closure  a DEVICE plane [P][W], 8-byte aligned (or CYC_ERR_ARG naming d_closure); exactly the plane's bytes are
 *              written, synchronously on the table's stream like cyc_table_adjacency's d_adj
 *   n_reach    host [P]: the set bits of row p (>= 1)
 * With P == 0 nothing is written and the call returns CYC_OK.
 * Device scratch of the call, freed before it returns: one closure plane of P rows of W words rounded up to 16, a pivot
 * panel of 64 such rows, one 64-bit word per pod (two with n_reach) and, for CYC_REACH_FROM, 16 bytes per (slot, word)
 * of the range; an allocation that fails is CYC_ERR_OOM with the byte count and what it was for.  The work is W steps
 * of two launches over that plane (a blocked Warshall, 64 pivots a step). */
int cyc_table_closure(cyc_table* t, int64_t k_lo, int64_t k_hi, int direction /* cyc_reach_direction */,
                      uint64_t* d_closure /* DEVICE [P][W], optional */, int64_t* n_reach /* host [P], optional */);
/* The zones of the table: pods p and q are in one zone iff each reaches the other (the strongly connected components
 * of the edges).  Zone ids are canonical like cyc_table_classes' class ids: zones are numbered 0, 1, ... in the order
 * of their smallest member pod, so zone[0] == 0.  Outputs (host, each optional, at least one, or CYC_ERR_ARG):
 *   zone     int32 [P]: the zone of every pod;  n_zones: the number of zones
 *   n_from   [P]: the pods that p reaches, itself included (the CYC_REACH_FROM closure's row count)
 *   n_to     [P]: the pods that reach p, itself included (its column count)
 * An empty slot range gives zone[p] = p, n_zones = P and all counts 1; with P == 0 only n_zones (0) is written.
 * Device scratch: cyc_table_closure's for CYC_REACH_FROM, and 20 bytes a pod. */
int cyc_table_zones(cyc_table* t, int64_t k_lo, int64_t k_hi, int32_t* zone, int64_t* n_zones,
                    int64_t* n_from /* host [P] */, int64_t* n_to /* host [P] */);
/* ---- How the zones are connected: the condensation of the reach graph (one node per zone) reduced to its Hasse
 * diagram, and the tier of every zone.  The reference has no such summary.  Edges, slot range, accepted tables and
 * their refusal text, stream, lifetime and plane alignment as for cyc_table_zones; nothing about the table, its
 * context, the options or cyc_last_* changes; the results are exact and the same from run to run.
 *
 * Z and the zone numbering are cyc_table_zones' (canonical by smallest member pod), so rep is ascending and
 * rep[0] == 0.  Zone a reaches zone b iff rep[a] reaches rep[b] in the CYC_REACH_FROM closure (reflexive); the strict
 * relation S drops the diagonal and is a strict partial order.  a -> b is a cover edge iff S[a][b] and no zone c has
 * S[a][c] and S[c][b].  Every cover edge is witnessed by a table edge from some pod of a to some pod of b; every other
 * edge between two zones is a shortcut the cover edges imply.  tier[z] is the number of edges of the longest chain of
 * cover edges that ends in z: 0 for a zone that no other zone reaches.
 *   zone      host int32 [P], optional: as cyc_table_zones;  n_zones: required, Z
 *   rep       host int32, room for P, optional: [z] = the smallest pod of zone z (the first Z are written)
 *   size      host int64, room for P, optional: [z] = the pods of zone z
 *   tier      host int32, room for P, optional
 *   edges     the cover edges in ascending (a, b) order.  *n_edges, when non-NULL, always receives their number.
 *             edges == NULL with edge_cap == 0 is a count-only call.  edges non-NULL with edge_cap below the number is
 *             CYC_ERR_ARG naming the number: *n_zones and *n_edges are set and nothing else is written.  edges without
 *             n_edges, a negative edge_cap, or NULL edges with edge_cap > 0: CYC_ERR_ARG.
 *   d_zreach  a DEVICE plane, optional: the reflexive zone reach matrix as tight rows [Z][Wz], Wz = ceil(Z / 64): row a
 *             bit b set iff a reaches b, bits at or beyond Z are 0.  8-byte aligned (or CYC_ERR_ARG naming d_zreach);
 *             exactly Z * Wz words are written, synchronously on the table's stream.  zreach_words < Z * Wz is
 *             CYC_ERR_ARG naming Z and the words needed: *n_zones is set and nothing else is written.
 * Apart from those two capacity failures outputs are written only on success.  An empty slot range gives Z = P,
 * zone[p] = rep[p] = p, sizes 1, tiers 0, no edge and the identity plane; with P == 0 only *n_zones = 0 and
 * *n_edges = 0 are written.  A NULL n_zones is CYC_ERR_ARG; a bad slot range or a partial table fails with
 * cyc_table_zones' messages.
 * Device scratch: cyc_table_zones', 4 bytes a zone, and as far as the outputs need them: the zone reach plane of Z
 * rows of Wz words rounded up to 16 (edges, tiers or d_zreach), a second such plane and 8 bytes a zone (edges or
 * tiers), 8 bytes an edge (a listing).  An allocation that fails is CYC_ERR_OOM with the byte count and what it was
 * for.  The work beyond cyc_table_zones' is a gather of the closure into the zone plane and one boolean product over it
 * in a single launch. */
typedef struct {
  int32_t a, b; /* zone a -> zone b, a != b */
} cyc_zone_edge;
int cyc_table_zone_graph(cyc_table* t, int64_t k_lo, int64_t k_hi, int32_t* zone /* host [P], optional */,
                         int64_t* n_zones, int32_t* rep, int64_t* size, int32_t* tier, cyc_zone_edge* edges,
                         int64_t edge_cap, int64_t* n_edges, uint64_t* d_zreach /* DEVICE, optional */,
                         int64_t zreach_words);
/* ---- Connectivity classes: the lossless summary of a table.  The reference prints every pod (table.go:58-156);
 * most pods of a real cluster behave exactly like many others, and the whole table is a class x class table
 * (cyc_table_cells_at over one representative per class) plus the two index arrays below.  Unlike the engine's
 * identity classes these are read off the table, so they exist for a wrapped table too and are as coarse as the
 * enforced behaviour.  The code of a cell is the code cyc_table_cells returns for `view` (a cyc_view) at (s, d, k),
 * CYC_CONN_NO_JOB included; the slot range is [k_lo, k_hi).
 *   source classes       pods p and q are in one class iff code(p, d, k) == code(q, d, k) for every destination d
 *                        in [0, P) and every k of the range
 *   destination classes  p and q are in one class iff code(s, p, k) == code(s, q, k) for every source s and every k
 * A non-VALID job's code depends on (d, k) only: it never separates sources, and it separates destinations exactly
 * when the status gives the view another code (under CYC_VIEW_EGRESS both invalid kinds are `unknown` and do not
 * separate; under the other two views they do).  Plane bits at or beyond P and plane bits of non-VALID (d, k)
 * never matter; loopback is not special.  Class ids are canonical: classes are numbered 0, 1, ... in the order of
 * their smallest member pod, so class[0] == 0, and the ids are the same from run to run.  An empty slot range puts
 * every pod in class 0 on both sides; with P == 0 nothing is written to the arrays and the counts are 0.
 * Outputs (host, each optional, at least one): src_class, dst_class int32 [P]; n_src, n_dst the numbers of classes.
 * Exactly the stated number of elements is written, and only when the call succeeds.  Accepted tables as for
 * cyc_table_reach (one that answers every cell; any other is refused with the text of a partial target-row table).
 * Stream, lifetime, plane alignment as for cyc_table_counts; the call changes neither the table, the context, its
 * options nor cyc_last_*.  CYC_ERR_ARG, each with its message: an unknown view, a bad slot range, all outputs NULL.
 * Rows are hashed on the device, grouped on the host and then compared word for word on the device, so the result
 * is exact whatever the hash does.  Device scratch of the call, freed before it returns: per side one bit plane of
 * P rows of W words rounded up to 16, 20 bytes a pod, and for sources 16 bytes per (slot, word); an allocation
 * that fails is CYC_ERR_OOM with the byte count. */
int cyc_table_classes(cyc_table* t, int view /* cyc_view */, int64_t k_lo, int64_t k_hi, int32_t* src_class,
                      int32_t* dst_class, int64_t* n_src, int64_t* n_dst);
/* Diagnostic twin: the row hash is ANDed with hash_mask before pods are grouped (0 groups by nothing but the
 * verification).  The four outputs above do not depend on hash_mask; cyc_table_classes is this call with ~0 and no
 * stats.  stats: optional host int64[4] = {verification rounds for sources, pods that failed a verification as
 * sources, the same two for destinations}. */
int cyc_table_classes_masked(cyc_table* t, int view /* cyc_view */, int64_t k_lo, int64_t k_hi, int32_t* src_class,
                             int32_t* dst_class, int64_t* n_src, int64_t* n_dst, uint64_t hash_mask, int64_t* stats);
/* cyc_table_cells for lists of pods instead of ranges (a class table is cells_at(representatives, representatives)):
 * out index ((i * n_d + j) * nk + k - k_lo) for srcs[i], dsts[j]; duplicates and any order allowed; an empty list
 * or slot range writes nothing.  The lists are host arrays, copied during the call.  Row requirements per output as
 * cyc_table_cells, for every listed pod.  CYC_ERR_ARG, each with its message: a bad slot range, a negative count, a
 * NULL list with a positive count, a list entry outside [0, P) (the message names the list, the first bad index and
 * its value), all outputs NULL.  Outputs are written only when the call succeeds. */
int cyc_table_cells_at(cyc_table* t, const int32_t* srcs, int64_t n_s, const int32_t* dsts, int64_t n_d, int64_t k_lo,
                       int64_t k_hi, uint8_t* ingress, uint8_t* egress, uint8_t* combined);
/* out[0..7] = pods, slots, words, row_lo, row_hi, partition, ingress window first word, window words */
int cyc_table_shape(const cyc_table* t, int64_t* out, int n);
const char* cyc_table_error(const cyc_table* t);
void cyc_table_destroy(cyc_table* t);

/* ---- Multi-GPU table assembly over RCCL (north_star: "Source-pod rows shard across the 8 GPUs of one
 * node, with an RCCL all-gather over xGMI only to assemble the final table").  One process per GPU,
 * each with its own context.  The shards need no exchange (cyc_probe_run_rows); a Go multi-GPU
 * Runner.RunProbeForConfig (pkg/connectivity/probe/jobrunner.go:29-31) that returns a whole *Table on
 * every rank assembles it with these.  Rank 0 makes the unique id, the host hands its 128 bytes to
 * every rank by its own means (e.g. over the same channel that started the ranks), and every rank
 * calls cyc_comm_init with it; the context owns the communicator until cyc_comm_destroy or
 * cyc_ctx_destroy.  RCCL failures return CYC_ERR_RCCL with RCCL's message. */
#define CYC_COMM_ID_BYTES 128 /* ncclUniqueId */
int cyc_comm_unique_id(uint8_t* id);  /* id: CYC_COMM_ID_BYTES bytes (needs no context) */
int cyc_comm_init(cyc_ctx* ctx, int nranks, int rank, const uint8_t* id);  /* collective over the ranks */
int cyc_comm_destroy(cyc_ctx* ctx);
/* The library's partition of the prepared pods over nranks: rank `rank`'s rows [*row_lo, *row_hi)
 * under `partition` (target rows balanced to a row; source rows to a 64-pod word).  The all-gathers
 * below assume every rank ran exactly these rows. */
int cyc_rows_shard(cyc_ctx* ctx, int partition, int nranks, int rank, int64_t* row_lo, int64_t* row_hi);
/* Collective: every rank passes its shard planes (cyc_probe_run_rows output for its cyc_rows_shard
 * rows, complete on `hip_stream` or before) and receives the whole [P][K][W] ingress and egress
 * planes (cyc_probe_run's layout over rows [0, P)) in d_ingress_full / d_egress_full, enqueued on
 * `hip_stream` (asynchronous).  Row shares move by grouped RCCL broadcasts straight into place (in
 * place when a shard already sits at its rows of the full plane); a source partition's ingress slices
 * are gathered in ~256 MB chunks and scattered into whole rows by a HIP kernel (two scratch buffers
 * the context keeps).  The status plane is whole on every rank already (cyc_probe_run_rows). */
int cyc_planes_allgather(cyc_ctx* ctx, void* hip_stream, int partition, const uint64_t* d_ingress,
                         const uint64_t* d_egress, uint64_t* d_ingress_full, uint64_t* d_egress_full);
/* Collective, on a device-resident table: `shard` is this rank's cyc_table_run_rows /
 * cyc_table_wrap_rows table for its cyc_rows_shard rows; *out becomes a whole table (target rows
 * [0, P), planes it owns) answering Table.Get(from, to) for every pair on every rank.  Synchronous. */
int cyc_table_allgather(cyc_ctx* ctx, const cyc_table* shard, cyc_table** out);
/* One GPU, no communicator: the whole ingress plane from all nranks source shards' ingress slices
 * (d_slices[r] = rank r's [P][K][Wr_r] plane for its cyc_rows_shard source rows) — the relayout step of
 * cyc_planes_allgather on its own (enqueued on hip_stream). */
int cyc_rows_merge_sources(cyc_ctx* ctx, void* hip_stream, int nranks, const uint64_t* const* d_slices,
                           uint64_t* d_ingress_full);

/* ---- Batched independent problems ("blocks", SURVEY §8f row 3: the generate sweep's many small
 * probe problems, interpreter.go:137-148, in one pass).  Resources.Pods is cut into consecutive pod
 * ranges: block b = pods [block_end[b-1], block_end[b]) answering probe config block_config[b] (an
 * index into probes_json) over its OWN pods only — its table is the one Runner.RunProbeForConfig
 * would build for that problem alone.  The caller gives every block its own namespaces (a block's
 * policies live in them; cyclonus_amd/batch.py prefixes "<b>~"), which the library checks: a
 * namespace with pods in two blocks is refused.  Only intra-block cells are computed and written:
 * each class row covers its block's 64-pod words only, and block b's output is a slab of
 *   ingress[d][k][j], egress[s][k][j]   (pods of the block, slots of its config, j < ceil(n_b/64)),
 *   status[d][k]
 * with bit i of word j = the block's pod 64*j + i; slab offsets from cyc_blocks_layout. */
int cyc_probe_prepare_blocks(cyc_ctx* ctx, const char* probes_json, size_t len, const int64_t* block_end,
                             const int32_t* block_config, int64_t n_blocks, cyc_probe_shape* shape);
/* out[2*b], out[2*b+1] = block b's plane slab offset (64-bit words) and status offset (bytes);
 * out[2*n_blocks], out[2*n_blocks+1] = the totals (n >= 2 * (n_blocks + 1)). */
int cyc_blocks_layout(cyc_ctx* ctx, int64_t* out, int64_t n);
/* Run every block (device slabs, synchronous only when an input can panic).  block_status[b] (host,
 * optional) = the cyc_status block b's stand-alone run would end with: CYC_OK, or the reference's
 * panic / table-build fatal for THAT problem (its first panicking job in its own job order), with
 * the message in cyc_block_error(ctx, b).  Other blocks are unaffected by one block's panic. */
int cyc_probe_run_blocks(cyc_ctx* ctx, void* hip_stream, uint64_t* d_ingress, uint64_t* d_egress, uint8_t* d_status,
                         int32_t* block_status);
const char* cyc_block_error(const cyc_ctx* ctx, int64_t block);

/* Average device time (ms) of the last run's kernels, measured with HIP events on the launch
 * stream: [0] whole pipeline, [1] the emit launch (the HBM-roofline kernel; one launch writes both
 * planes), [2] class rows of both directions.  Eager runs ("graphs" = 0) always record them; graph
 * and fused-eager runs only with "step_events" = 1, and report only [0] ([1], [2] = -1); without
 * events the call fails with CYC_ERR_ARG.
 * cyc_last_timings, cyc_last_classes and cyc_last_emit answer for runs of the current prepare only:
 * after a cyc_probe_prepare* and before the next run they fail with CYC_ERR_ARG ("no run yet"), and
 * "row_phases_active" reads 0. */
int cyc_last_timings(cyc_ctx* ctx, double* ms, int n);

/* Diagnostic: number of distinct classes (class rows computed) of the last run, [0] ingress,
 * [1] egress (synchronises the stream the last run was enqueued on, which must still exist). */
int cyc_last_classes(cyc_ctx* ctx, int64_t* out, int n);

/* What the last enqueued run's emit launched: the kernel name(s) ("k_emit_wide_buf<512,13>",
 * "k_emit_units<1024,7>", ...; several joined by " + ") into name (NUL-terminated, truncated to
 * cap - 1 bytes) and the number of emit launches into *launches (either may be null).  Set when the
 * run is enqueued (a captured graph replays what its capture recorded); CYC_ERR_ARG before any run. */
int cyc_last_emit(cyc_ctx* ctx, char* name, size_t cap, int64_t* launches);

/* Diagnostic path selectors (results never change; the GPU tests force every path):
 *   "graphs"      -1 (default: auto = 2 when the fused front applies, else 1); 1 replays the step as
 *                 one captured hipGraph when the inputs cannot panic (then cyc_last_timings reports
 *                 only the whole-pipeline time); 2 enqueues the same launches eagerly (the fused
 *                 front on the caller's stream, or the three-stream DAG); 0 runs every kernel in
 *                 order on the caller's stream with per-phase events
 *   "front_fused" 1 (default): the front as block-range-fused launches on one stream, one per
 *                 dependency level (no-panic builds with dense selectors); 0: the two-branch DAG
 *   "pod_words"   -1 (default: auto) / 0 / 1: class rows read pod-peer words from materialised peer
 *                 rows (0) or expand them from per-identity outcomes through each word's identity
 *                 runs (1, needs <= 4 runs per word and no possible panic)
 *   "pod_rows"    -1 (default: auto = 1 when identities >= pods / 2) / 0 / 1: materialised pod-peer
 *                 rows through identity outcomes and word runs (0) or per pod (1)
 *   "member_wave" -1 (default: auto = 1 for <= 4096 identities) / 0 / 1: target membership with a
 *                 thread (0) or a wave (1) per pod identity
 *   "class_rpb"   0 (default: auto) / 1..64: class representatives per identity-set class-row block
 *   "step_events" 0 (default) / 1: graph and fused-eager runs also record the whole-step timing
 *                 events cyc_last_timings reads (they idle the GPU ~9 us between steps)
 *   "pl_wave"     1 (default) / 0: materialised-row class rows a wave per 64-word chunk where they
 *                 fit (<= 4 job slots and descriptors), or a thread per (slot chunk, word) item
 *   "pr_group"    -1 (default: auto) / 1..64: the fused front's sparse pod-peer rows (PM builds) with
 *                 a block per pod peer (1) or a wave per 64-word chunk over groups of that many peers
 *   "class_inplace" -1 (default: auto) / 0 / 1: on the fused front, each class's rows are written
 *                 straight into the output planes at its first member pod's row and the emit copies
 *                 them to the class's other pods (1), or they go to a buffer of their own the emit
 *                 copies from (0); auto = 1 when the rows' identities are >= 1/16 of the rows or
 *                 the run is an identity-set build
 *   "sel_lazy"    -1 (default: auto) / 0 / 1: on the fused front, label selectors are evaluated where
 *                 membership and pod-peer rows / identity sets use them (1) instead of as the dense
 *                 selector x label-set table first (0); auto = 1 for identity-set builds and once
 *                 that table has >= 64M pairs
 *   "ip_range"    -1 (default: auto = where the words' addresses are not affine) / 0 / 1: IP rows of
 *                 few, close pods built from the address index wherever they fit (1), or never (0)
 *   "ip_iv"       -1 (default: auto) / 0: IP rows as pod-index intervals where the network's family holds
 *                 non-decreasing addresses in pod order (ip_rows_iv_blk), or through the paths below
 *   "ip_items"    -1 (default: auto = 1 for runs over every row) / 0 / 1: the fused front's IP rows as
 *                 per-chunk work items of the rows that touch each chunk (1) or as groups of 16 rows a
 *                 wave over 4 chunks (0)
 *   "emit_interleave" -1 (default: auto = 1 when a plane of a target-row run is >= 8 GB) / 0 / 1: the
 *                 emit's row list alternates ingress and egress rows (1) or holds all ingress rows first
 *   "row_phases"  -1 (default: auto = 2 for whole no-panic tables whose planes are >= 8 GB) / 1 / 2: the
 *                 class rows and the emit in two row phases (the classes rows [0, P/2) use, those rows'
 *                 emit, then the other classes and rows [P/2, P)) or in one pass (1); the fused front
 *                 runs once either way (phase 1's emit on a second stream under phase 2's class rows
 *                 was 4-7 % slower: profiles/r06_row_phases_ab.txt)
 *   "plvt_max_mb" 1024 (default) / 0..1048576: the largest per-pod label table (PLVT) the sparse pod-peer
 *                 rows build on the device; beyond it (0: always) they gather through each pod's label set
 * cyc_get_option also reports "launch" (the graphs mode in effect), "row_phases_active" (the last
 * run's phases: 2, or 0), "front_fused_active", "pl_wave_active", "port_bits_active" (the port table's
 * descriptor bit rows: at most 32 descriptors), "slot_words_active" (the slot words are built) and
 * "uni_desc_active" (every pod has the same VALID descriptor in each slot; these four need cyc_probe_prepare),
 * "class_inplace_active" and "emit_interleave_active" (the routes in effect; they need a run),
 * "plvt_active", "ip_iv_rows" and "ip_range_rows" (the current range plan's
 * interval-built and range-built IP rows), "pod_post_rows" and "pod_scan_rows" (its sparse pod-peer rows built
 * from label postings and by scanning the pods; both 0 unless the route in effect builds sparse pod-peer rows:
 * the fused front of a materialised-row build); "pod_words" reports the mode the prepared probe uses (0 or 1; needs
 * cyc_probe_prepare).  Of the last cyc_probe_target_effects call it reports "effects_batches" (class batches),
 * "effects_launches" (allow-row builds: one per batch and word window) and "effects_scratch_bytes" (device
 * bytes it held at its peak), and "effects_scratch_cap" reports the bytes its batch buffers may take (256 MB). */
int cyc_set_option(cyc_ctx* ctx, const char* name, int64_t value);
int cyc_get_option(cyc_ctx* ctx, const char* name, int64_t* value);

/* Single-cell API (policy.go:131-174): traffic_json is a JSON array of matcher.Traffic objects;
 * out[i] = ingress | egress << 1 (allowed bits).  Needs only a loaded policy. */
int cyc_query_traffic(cyc_ctx* ctx, const char* traffic_json, size_t len, uint8_t* out, int64_t n);

/* matcher.Traffic values (pkg/matcher/traffic.go:11-18) as flat tables, the form a cgo
 * SimulatedJobRunner.RunJobs over explicit []*Job (jobrunner.go:68-94, Job.Traffic job.go:81-103)
 * passes without JSON.  Endpoint 2i is traffic i's Source, 2i + 1 its Destination; an endpoint is
 * internal when internal[e] is 1 (TrafficPeer.Internal != nil: its namespace, pod labels and
 * namespace labels are read), external otherwise (only its IP).  A nil label map is given as an
 * empty range (the matchers read nil and empty maps alike); label_off / ns_label_off may be NULL
 * when no endpoint has labels. */
typedef struct {
  cyc_strings str;
  int64_t n;                         /* traffics */
  const uint8_t* internal;           /* [2n] */
  const int32_t* ip;                 /* [2n] TrafficPeer.IP */
  const int32_t* ns;                 /* [2n] Internal.Namespace (internal endpoints) */
  const int64_t* label_off;          /* [2n + 1] into label_key / label_val: Internal.PodLabels */
  const int32_t *label_key, *label_val;
  const int64_t* ns_label_off;       /* [2n + 1] into ns_label_key / ns_label_val: Internal.NamespaceLabels */
  const int32_t *ns_label_key, *ns_label_val;
  const int32_t* port;               /* [n] ResolvedPort */
  const int32_t* port_name;          /* [n] ResolvedPortName */
  const int32_t* protocol;           /* [n] Protocol (the raw string) */
} cyc_traffic_tables;
/* cyc_query_traffic over flat tables: out[i] = ingress | egress << 1; panics as cyc_query_traffic. */
int cyc_query_traffic_tables(cyc_ctx* ctx, const cyc_traffic_tables* tables, uint8_t* out, int64_t n);

/* query-traffic with the DirectionResult target lists (replaces Policy.IsTrafficAllowed's
 * AllowedResult, policy.go:84-96,131-174, as printed by analyze.go:209-225).  out_json gets a
 * JSON array, one object per traffic:
 *   {"Ingress": {"AllowingTargets": [pk, ...], "DenyingTargets": [pk, ...], "IsAllowed": b},
 *    "Egress": {...}, "IsAllowed": b}
 * pk = the target's primary key (target.go:57-62, the key of Policy.Ingress / Policy.Egress).
 * Lists are in primary-key order (Go walks the target map in random order).  *needed = bytes
 * required incl. the NUL; CYC_ERR_ARG when cap is smaller.  Panics as cyc_query_traffic. */
int cyc_query_traffic_targets(cyc_ctx* ctx, const char* traffic_json, size_t len, char* out_json, size_t cap,
                              size_t* needed);

/* query-target (analyze.go:163-204 QueryTargets / QueryTargetHelper): pods_json is a JSON list
 * of {"Namespace": ns, "Labels": {...}} (QueryTargetPod); out_json gets, per pod,
 * {"Ingress": [pk, ...], "Egress": [pk, ...]} = Policy.TargetsApplyingToPod (policy.go:68-82) per
 * direction, in primary-key order.  An invalid selector operator panics ("invalid operator"). */
int cyc_query_targets(cyc_ctx* ctx, const char* pods_json, size_t len, char* out_json, size_t cap, size_t* needed);

#ifdef __cplusplus
}
#endif
#endif /* CYCLONUS_HIP_H */
