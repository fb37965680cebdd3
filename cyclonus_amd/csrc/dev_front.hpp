// dev_front.hpp — the fused front: launches A-E as concatenations of the per-block bodies above.
// Part of engine.hip's single translation unit (device bodies inline across stages, host helpers are
// static): included once, by engine.hip, in stage order.
#pragma once

namespace cyc {

// Fused front (cyc_set_option "front_fused", IDO builds): the front's ~15 kernels of two graph
// branches become 5 launches on ONE stream, each launch a concatenation of independent block
// ranges (every range calls the same per-block body as its stand-alone kernel, with its own
// block index and count).  A launch depends on the previous one only, so the graph needs no
// cross-stream edges (each cost ~10 us of join latency on the critical path) and both
// directions' blocks share every launch.
//   A: IP word spans reset | port table | slot words | selectors        (independent)
//   B: IP rows (both directions) | pod-peer identity sets (both) | membership in | membership eg
//      (membership dispatched first unless the IP rows fill the chip: FrontB::member_first)
//   C: class election in | eg           D: identity sets in | eg         E: class rows in | eg
// Every launch holds its stages' own argument structs (each defined next to its *_blk body, filled by
// its host builder in enqueue.hpp) and hands its blocks out in the order of the take() calls below.
__device__ __forceinline__ bool take(uint32_t& b, uint32_t nb) {  // block b in the next nb blocks? else past them
  if (b < nb) return true;
  b -= nb;
  return false;
}
struct FrontA {
  FillArgs fill;
  PortArgs port_table;
  SlotWordsArgs slot_words;
  SelArgs sel;
  uint64_t blocks() const { return uint64_t(fill.nb) + port_table.nb + slot_words.nb + sel.nb; }
};
__global__ __launch_bounds__(256) void k_front_a(FrontA f) {
  uint32_t b = blockIdx.x;
  if (take(b, f.fill.nb)) return fill_u32_blk(f.fill, b);
  if (take(b, f.port_table.nb)) return portok_blk(f.port_table, b);
  if (take(b, f.slot_words.nb)) return slot_words_blk(f.slot_words, b);
  if (take(b, f.sel.nb)) selectors_dense_blk(f.sel, b);
}

// Peer rows are built over a word window per direction: a source shard's ingress peers only over
// its sources' words (chunks [c0, c0 + nch)), everything else over all words.  Segment x of the IP
// rows and of the per-pod pod-peer rows is one direction's sub-list (target-row runs put both
// directions into segment 0: one window).
struct MemberSeg {
  uint32_t nb, wave;  // wave 1: a wave per identity (k_member_wave), 0: a thread per identity
  MemberArgs a;
};
struct FrontB {
  PeerCommon pc;
  IpIvArgs ip_iv[2];        // IP rows as pod intervals
  IpArgs ip[2];             // IP rows per word (groups or work items)
  IpRangeArgs ip_range[2];  // IP rows from address ranges
  PodDirectArgs pods[2];    // PM builds with few pod-peer words: full pod-peer rows per pod, or
  IdentArgs ident[2];       // IDO builds: identity sets per direction
  MemberSeg member[2];
  // membership blocks dispatched first (1) or after the pod-peer rows (0): few blocks, each a chain
  // of dependent loads, which first start at once instead of waiting for slots behind thousands of
  // short pod-row blocks (config #2: B 23.1 -> 16.5 us); behind a chip-full of IP rows they go last,
  // filling the tail instead of holding slots the IP rows need (config #4: first 66.6, last 64.1 us)
  uint32_t member_first;
  PortBitsArgs port_bits;    // for the identity sets and the class rows
  PortArgs port_table;       // the port table and slot words of runs without launch A (build_front)
  SlotWordsArgs slot_words;
  uint64_t blocks() const {
    uint64_t n = uint64_t(port_bits.nb) + port_table.nb + slot_words.nb;
    for (int x = 0; x < 2; x++) n += uint64_t(ip_iv[x].nb) + ip[x].nb + ip_range[x].nb + pods[x].nb + ident[x].nb + member[x].nb;
    return n;
  }
};
__device__ __forceinline__ bool front_b_member(const FrontB& f, uint32_t& b) {
#pragma unroll
  for (int d = 0; d < 2; d++)
    if (take(b, f.member[d].nb)) {
      if (f.member[d].wave) member_wave_blk(f.member[d].a, b, f.member[d].nb);
      else member_blk(f.member[d].a, b, f.member[d].nb);
      return true;
    }
  return false;
}
__global__ __launch_bounds__(256) void k_front_b(FrontB f) {
  uint32_t b = blockIdx.x;
  if (f.member_first && front_b_member(f, b)) return;
#pragma unroll
  for (int x = 0; x < 2; x++)
    if (take(b, f.ip_iv[x].nb)) return ip_rows_iv_blk(f.pc, f.ip_iv[x], b);
#pragma unroll
  for (int x = 0; x < 2; x++)
    if (take(b, f.ip[x].nb)) return f.ip[x].items ? ip_rows_items_blk(f.pc, f.ip[x], b) : ip_rows_fast_blk(f.pc, f.ip[x], b);
#pragma unroll
  for (int x = 0; x < 2; x++) {
    if (take(b, f.pods[x].nb)) return pod_rows_direct_blk<false, true>(f.pc, f.pods[x], b);
    if (take(b, f.ident[x].nb)) return peer_bits_blk(f.pc, f.ident[x], b);
  }
  if (!f.member_first && front_b_member(f, b)) return;
  if (take(b, f.port_bits.nb)) return f.port_bits.direct ? portbits_direct_blk(f.port_bits, b) : portbits_blk(f.port_bits, b);
  if (take(b, f.port_table.nb)) return portok_blk(f.port_table, b);
  if (take(b, f.slot_words.nb)) return slot_words_blk(f.slot_words, b);
#pragma unroll
  for (int x = 0; x < 2; x++)
    if (take(b, f.ip_range[x].nb)) return ip_rows_range_blk(f.pc, f.ip_range[x], b);
}

// Pod-peer rows from posting lists: a pod selector that is ONE requirement `k = v` or `k in (v0,
// v1)` (matchLabels, the common shape) matches exactly the pods listed under (k, v) in the host's
// label postings, so its row is built from those few pods instead of testing every pod: block =
// one such peer; the row is assembled in LDS PR_POST_WORDS words at a time (each pod of the
// postings whose namespace the peer's namespace matcher accepts sets its bit with an LDS atomic
// OR), then stored chunk-dense with span and chunk masks (pod_chunk_store).  Cost ~ postings +
// nonzero chunks, not pods.
constexpr uint32_t PR_POST_WORDS = 1024;  // 16 chunks of the row per LDS pass (8 KB)
__device__ __forceinline__ void pod_rows_post_blk(const PeerCommon& cm, const PodSparseArgs& a, uint32_t bid_) {
  const uint32_t W = cm.W, c0 = a.c0, nch = a.nch;
  const SelView& sv = cm.sv;
  __shared__ unsigned long long s_row[PR_POST_WORDS];
  const uint32_t j = a.plist_post[bid_];
  const DPeer pr = cm.peers[j];
  const uint4 pp = cm.req_post[sv.sel_off[pr.podsel]];  // (offset, count) of value 0, then of value 1
  // chunks [c0, c0 + nch) of the row (a source shard's ingress peers: the chunks of its word window)
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, chunks = c0 + nch;
  for (uint32_t w0 = c0 * 64; w0 < min(W, chunks * 64); w0 += PR_POST_WORDS) {
    for (uint32_t x = threadIdx.x; x < PR_POST_WORDS; x += blockDim.x) s_row[x] = 0;
    __syncthreads();
    for (uint32_t e = threadIdx.x; e < pp.y + pp.w; e += blockDim.x) {
      const uint32_t q = cm.post_pods[e < pp.y ? pp.x + e : pp.z + (e - pp.y)];
      const uint32_t w = q >> 6;
      if (w < w0 || w >= w0 + PR_POST_WORDS) continue;
      bool ok = pr.nskind == 1;  // podpeermatcher.go:21-28: the namespace matcher
      if (pr.nskind == 0) ok = cm.pod_ns[q] == pr.nsval;
      else if (pr.nskind == 2) ok = sel_at(sv, pr.nsval, cm.pod_nsls[q]) == 1;
      if (ok) atomicOr(&s_row[w - w0], 1ull << (q & 63));
    }
    __syncthreads();
    for (uint32_t c = w0 / 64 + wave; c < min(chunks, (w0 + PR_POST_WORDS) / 64); c += blockDim.x >> 6)
      pod_chunk_store(j, c, W, lane, c * 64 + lane < W ? s_row[c * 64 + lane - w0] : 0ull, cm.PM, cm.rng, cm.cnz);
    __syncthreads();  // s_row is cleared for the next pass
  }
}

// Launch C also carries PM builds' sparse pod-peer rows (they need only launch A's selector table
// and precede the class rows): the light class election keeps them off launch B, whose IP rows and
// membership would otherwise run at the pod rows' register budget (occupancy 8 -> 5-7).
struct ElectSeg {
  uint32_t nb;
  MemberArgs a;
  uint32_t* class_of;
};
struct FrontC {
  ElectSeg elect[2];  // class election in | eg
  // sparse pod-peer rows (pod_rows_sparse_blk over plist, then pod_rows_post_blk over plist_post),
  // one segment per word window (ingress peers of a source shard / the rest)
  PeerCommon pc;
  PodSparseArgs pods[2];
  uint64_t blocks() const {
    uint64_t n = 0;
    for (int x = 0; x < 2; x++) n += uint64_t(elect[x].nb) + pods[x].nb + pods[x].nb_post;
    return n;
  }
};
__global__ __launch_bounds__(256) void k_front_c(FrontC f) {
  uint32_t b = blockIdx.x;
#pragma unroll
  for (int d = 0; d < 2; d++)
    if (take(b, f.elect[d].nb)) return classify_blk(f.elect[d].a, f.elect[d].class_of, b, f.elect[d].nb);
#pragma unroll
  for (int x = 0; x < 2; x++)
    if (take(b, f.pods[x].nb)) return pod_rows_sparse_blk(f.pc, f.pods[x], b);
#pragma unroll
  for (int x = 0; x < 2; x++)
    if (take(b, f.pods[x].nb_post)) return pod_rows_post_blk(f.pc, f.pods[x], b);
}
// The launch structs are kernel arguments: 4096 bytes is the limit.
static_assert(sizeof(FrontA) <= 4096 && sizeof(FrontB) <= 4096 && sizeof(FrontC) <= 4096, "kernel-argument limit");

struct FrontRows {
  uint32_t nb_in, nb_eg;
  RowArgs ra[2];
  __host__ __device__ uint32_t& nb(int d) { return d ? nb_eg : nb_in; }
};
static_assert(sizeof(FrontRows) <= 4096, "kernel-argument limit");
__global__ __launch_bounds__(256) void k_front_d(FrontRows f) {
  const uint32_t b = blockIdx.x;
  if (b < f.nb_in) class_ident_blk<false, CI_G>(f.ra[0], b, f.nb_in);
  else class_ident_blk<true, CI_G>(f.ra[1], b - f.nb_in, f.nb_eg);
}
// PM builds (pod-peer words from materialised rows): the class rows, egress blocks first
template <bool WAVE>
__global__ __launch_bounds__(256) void k_front_d_pm(FrontRows f) {
  __shared__ PlShared sh;
  const uint32_t b = blockIdx.x;
  if (b < f.nb_eg) class_rows_pl_blk<true, WAVE>(f.ra[1], sh, b, f.nb_eg);
  else class_rows_pl_blk<false, WAVE>(f.ra[0], sh, b - f.nb_eg, f.nb_in);
}

// egress blocks first: they are the slower ones (per-destination port masks), so the launch's
// tail is made of the shorter ingress blocks (4 job slots per thread: profiles/r01_front_e_kc_ab.txt)
constexpr int E_KC = 4;  // job slots per thread in the IDO class rows of the fused front
// Launch E as one kernel when the egress rows take the one-descriptor-per-slot form (UNI): both
// bodies then stay near 60 VGPRs, so the fused launch keeps their occupancy and saves a launch.
__global__ __launch_bounds__(256) void k_front_e_uni(FrontRows f) {
  uint32_t b = blockIdx.x;
  const bool eg = b < f.nb_eg;
  if (!eg) b -= f.nb_eg;
  if (eg) class_rows_ido_blk<true, E_KC, true>(f.ra[1], b, f.nb_eg);
  else class_rows_ido_blk<false, E_KC>(f.ra[0], b, f.nb_in);
}

}  // namespace cyc
