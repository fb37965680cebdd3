// dev_effects.hpp — which target decides: per-target effect counts over the verdict grid (cyc_probe_target_effects).
// Part of engine.hip's single translation unit (device bodies inline across stages, host helpers are
// static): included once, by engine.hip, in stage order.
//
// Policy.IsIngressOrEgressAllowed (policy.go:138-174) sorts every target applying to a cell's target pod
// into DirectionResult.AllowingTargets or .DenyingTargets (policy.go:84-96).  Nothing here walks cells: a
// target's allow row a[t][j] is a bit row over the peer pods for job descriptor j, and every count is a
// population count of such rows, multiplied by the number of target pods that share them.
#pragma once

namespace cyc {

// The bytes a call's batch buffers (allow rows, their counts) may take; the host batches classes, and
// windows the words of a batch that alone would not fit (engine.hip, cyc_probe_target_effects).
constexpr uint64_t EFF_SCRATCH_CAP = 256ull << 20;

// The prepared tables the kernels read (Prepared: filled by a prepare, never by a run).
struct EffTables {
  uint32_t P, K, W, D;
  const uint32_t *pod_ns, *pod_ls, *pod_nsls;
  const DIP* pod_ip;
  const uint32_t *sel_off, *req_vals, *ls_off, *ls_key, *ls_val;
  const DReq* reqs;
  const DPeer* peers;
  const DIPBlock* ipbs;
  const DCidr* cidrs;
  const uint32_t* ipb_ex;
  const DTarget* tgt;              // of the direction
  const uint32_t *tns_lo, *tns_hi;
  const int32_t* slot_desc;        // [P][K]
  const uint8_t* slot_status;
  const uint8_t* portok;           // [M][D], the call's own (k_portok)
};

__device__ __forceinline__ uint8_t eff_sel(const EffTables& x, uint32_t sel, uint32_t ls) {
  return eval_selector(x.sel_off, x.reqs, x.req_vals, x.ls_off, x.ls_key, x.ls_val, sel, ls);
}

__device__ __forceinline__ uint64_t eff_wave_sum(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down((unsigned long long)v, o);
  return v;  // lane 0 holds the sum
}
// Sum over a 256-thread block, returned to every thread (two barriers: the scratch may be reused at once).
__device__ __forceinline__ uint64_t eff_block_sum(uint64_t v, uint64_t* sh) {
  v = eff_wave_sum(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  const uint64_t s = sh[0] + sh[1] + sh[2] + sh[3];
  __syncthreads();
  return s;
}

// ---------------------------------------------------------------- TargetsApplyingToPod per (namespace, label set)
// policy.go:68-82 for every distinct (namespace, label set) of the rows' pods, a wave per identity: the
// targets of its namespace, 64 at a time, one selector evaluation per lane.  First the counts, then (FILL)
// the lists in primary-key order at the offsets the host summed.
struct EffMemberArgs {
  EffTables x;
  uint32_t n;
  const uint32_t *id_ns, *id_ls, *off;
  uint32_t *cnt, *list;
};
template <bool FILL>
__global__ __launch_bounds__(256) void k_eff_member(EffMemberArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  for (uint64_t i0 = blockIdx.x * 4ull + (threadIdx.x >> 6); i0 < a.n; i0 += gridDim.x * 4ull) {
    const uint32_t i = __builtin_amdgcn_readfirstlane(uint32_t(i0));
    const uint32_t ns = a.id_ns[i], ls = a.id_ls[i];
    const uint32_t lo = a.x.tns_lo[ns], hi = a.x.tns_hi[ns];
    uint32_t n = 0;
    for (uint32_t t0 = lo; t0 < hi; t0 += 64) {
      const uint32_t t = t0 + lane;
      const bool m = t < hi && eff_sel(a.x, a.x.tgt[t].sel, ls) == 1;
      const uint64_t b = __ballot(m);
      if (FILL && m) a.list[a.off[i] + n + __popcll(b & ((1ull << lane) - 1))] = t;
      n += __popcll(b);
    }
    if (!FILL && lane == 0) a.cnt[i] = n;
  }
}

// ---------------------------------------------------------------- egress: VALID pods per (slot, descriptor, word)
// V[kk][j][w]: bit q set when pod w * 64 + q has a VALID job in slot k_lo + kk with descriptor j (the
// descriptor of an egress cell belongs to its destination).  A wave per (slot, word).
struct EffValidArgs {
  EffTables x;
  uint32_t k_lo, nk;
  uint64_t* V;  // [nk][D][W]
};
__global__ __launch_bounds__(256) void k_eff_valid(EffValidArgs a) {
  const uint32_t lane = threadIdx.x & 63, W = a.x.W, D = a.x.D;
  const uint64_t n = uint64_t(a.nk) * W;
  for (uint64_t i0 = blockIdx.x * 4ull + (threadIdx.x >> 6); i0 < n; i0 += gridDim.x * 4ull) {
    const uint32_t kk = uint32_t(i0 / W), w = uint32_t(i0 % W), q = w * 64 + lane;
    int32_t e = -1;
    if (q < a.x.P && a.x.slot_status[uint64_t(q) * a.x.K + a.k_lo + kk] == CYC_JOB_VALID)
      e = a.x.slot_desc[uint64_t(q) * a.x.K + a.k_lo + kk];
    for (uint32_t j = 0; j < D; j++) {
      const uint64_t b = __ballot(e == int32_t(j));
      if (lane == 0) a.V[(uint64_t(kk) * D + j) * W + w] = b;
    }
  }
}

// ---------------------------------------------------------------- allow rows of a batch of targets
// a[tl][j][wl] = OR over the peers p of target tlist[tl] with portok[p.port][j] of p's match word over the
// pods of word w0 + wl (Target.Allows, target.go:29-36; PeerMatcher.Allows per kind).  A wave per (target,
// word): each lane evaluates its pod once per peer (podpeermatcher.go:21-28 / ippeermatcher.go:43-50), the
// ballot is the peer's word, and lane j keeps descriptor j's row word (the peer's word is formed once for
// the first 64 descriptors, again per further 64).  AllPeers and PortsForAllPeers are constant words.
struct EffRowArgs {
  EffTables x;
  uint32_t U, w0, WA;
  const uint32_t* tlist;  // [U] targets of the batch
  uint64_t* a;            // [U][D][WA]
};
__global__ __launch_bounds__(256) void k_eff_rows(EffRowArgs a) {
  const uint32_t lane = threadIdx.x & 63, D = a.x.D, P = a.x.P;
  const uint64_t n = uint64_t(a.U) * a.WA;
  for (uint64_t i0 = blockIdx.x * 4ull + (threadIdx.x >> 6); i0 < n; i0 += gridDim.x * 4ull) {
    const uint32_t tl = __builtin_amdgcn_readfirstlane(uint32_t(i0 / a.WA));
    const uint32_t wl = __builtin_amdgcn_readfirstlane(uint32_t(i0 % a.WA));
    const uint32_t w = a.w0 + wl, q = w * 64 + lane;
    const uint64_t full = uint64_t(w) * 64 + 64 <= P ? ~0ull : (1ull << (P - w * 64)) - 1;  // (w < W: 1..63 pods)
    const bool in = q < P;
    const uint32_t qc = in ? q : 0;
    const uint32_t ns = a.x.pod_ns[qc], nsls = a.x.pod_nsls[qc], ls = a.x.pod_ls[qc];
    const DTarget tg = a.x.tgt[a.tlist[tl]];
    const uint32_t p0 = __builtin_amdgcn_readfirstlane(tg.poff), p1 = p0 + __builtin_amdgcn_readfirstlane(tg.pcnt);
    for (uint32_t jc = 0; jc < D; jc += 64) {
      const uint32_t j = jc + lane;
      uint64_t acc = 0;
      for (uint32_t p = p0; p < p1; p++) {
        const DPeer pr = a.x.peers[p];
        const uint32_t kind = __builtin_amdgcn_readfirstlane(pr.kind);
        if (kind == 0) {  // AllPeersMatcher
          acc = full;
          break;
        }
        const bool pok = j < D && a.x.portok[uint64_t(pr.port) * D + j] != 0;
        if (kind == 1) {  // PortsForAllPeersMatcher
          acc = pok ? full : acc;
          continue;
        }
        bool m = false;
        if (in) {
          if (kind == 2) {
            m = pr.nskind == 1 || (pr.nskind == 0 ? ns == pr.nsval : eff_sel(a.x, pr.nsval, nsls) == 1);
            if (m && pr.podsel != CYC_ALL) m = eff_sel(a.x, pr.podsel, ls) == 1;
          } else {
            m = ip_peer_outcome(a.x.ipbs[pr.ipb], a.x.cidrs, a.x.ipb_ex, a.x.pod_ip[q]) == 1;
          }
        }
        const uint64_t word = __ballot(m);
        acc |= pok ? word : 0ull;
      }
      if (j < D) a.a[(uint64_t(tl) * D + j) * a.WA + wl] = acc;
    }
  }
}

// ---------------------------------------------------------------- ALLOWING: population counts of the rows
// Ingress (EG false): pop[tl][j] = bits of a[tl][j] in the window; the host multiplies by the pods of each
// class whose slot holds descriptor j.  Egress: pop[tl][kk] = sum over j of bits of a[tl][j] & V[kk][j].
// A block per output element.
struct EffPopArgs {
  uint32_t D, W, w0, WA, X;  // X outputs per target: D (ingress), slots (egress)
  const uint64_t *a, *V;
  unsigned long long* pop;  // ingress [U][D], egress [U][nk]
};
template <bool EG>
__global__ __launch_bounds__(256) void k_eff_pop(EffPopArgs a) {
  __shared__ uint64_t sh[4];
  const uint32_t tl = blockIdx.x / a.X, x = blockIdx.x % a.X;
  uint64_t s = 0;
  if (!EG) {
    const uint64_t* row = a.a + (uint64_t(tl) * a.D + x) * a.WA;
    for (uint32_t wl = threadIdx.x; wl < a.WA; wl += 256) s += __popcll(row[wl]);
  } else {
    for (uint32_t j = 0; j < a.D; j++) {
      const uint64_t* row = a.a + (uint64_t(tl) * a.D + j) * a.WA;
      const uint64_t* v = a.V + (uint64_t(x) * a.D + j) * a.W + a.w0;
      for (uint32_t wl = threadIdx.x; wl < a.WA; wl += 256) s += __popcll(row[wl] & v[wl]);
    }
  }
  s = eff_block_sum(s, sh);
  if (threadIdx.x == 0) a.pop[blockIdx.x] = s;
}

// ---------------------------------------------------------------- SOLE_ALLOWING: classes of two or more targets
// A class is the target pods of the rows with one set of applying targets (ingress: and one descriptor
// per slot).  Per (class, slot, 256-word chunk), a word per thread: sweep the class's targets with
// twos |= ones & a, ones |= a; ones & ~twos are the peers exactly one target allows, and a[t] & that
// attributes them.  Counts are multiplied by the class's pods and leave the block as one 64-bit atomicAdd
// per (target, slot).
struct EffSoleArgs {
  uint32_t D, W, w0, WA, nk, NC;
  const uint64_t *a, *V;
  const uint32_t *cls_off, *cls_t, *cls_n;  // class -> its targets (batch-local), its pods in the rows
  const int32_t* cls_desc;                  // ingress [NC][nk]: the class's VALID descriptor, or -1
  unsigned long long* sole;                 // [U][nk]
};
template <bool EG>
__device__ __forceinline__ uint64_t eff_allow_word(const EffSoleArgs& a, uint32_t tl, uint32_t kk, int32_t j, uint32_t wl) {
  if (!EG) return a.a[(uint64_t(tl) * a.D + uint32_t(j)) * a.WA + wl];
  uint64_t r = 0;
  for (uint32_t e = 0; e < a.D; e++) {
    const uint64_t v = a.V[(uint64_t(kk) * a.D + e) * a.W + a.w0 + wl];
    if (v) r |= v & a.a[(uint64_t(tl) * a.D + e) * a.WA + wl];
  }
  return r;
}
constexpr uint32_t EFF_TCH = 64;  // targets per reduction round
template <bool EG>
__global__ __launch_bounds__(256) void k_eff_sole(EffSoleArgs a) {
  __shared__ uint64_t part[4][EFF_TCH];
  const uint32_t chunks = (a.WA + 255) / 256, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t n = uint64_t(a.NC) * a.nk * chunks;
  for (uint64_t it = blockIdx.x; it < n; it += gridDim.x) {  // (block-uniform: barriers inside)
    const uint32_t ch = uint32_t(it % chunks), kk = uint32_t(it / chunks % a.nk), c = uint32_t(it / chunks / a.nk);
    const int32_t j = EG ? 0 : a.cls_desc[uint64_t(c) * a.nk + kk];
    if (j < 0) continue;  // the class's pods have no VALID job in this slot
    const uint32_t t0 = a.cls_off[c], t1 = a.cls_off[c + 1];
    const uint32_t wl = ch * 256 + threadIdx.x;
    const bool act = wl < a.WA;
    uint64_t ones = 0, twos = 0;
    for (uint32_t x = t0; x < t1; x++) {
      const uint64_t w = act ? eff_allow_word<EG>(a, a.cls_t[x], kk, j, wl) : 0ull;
      twos |= ones & w;
      ones |= w;
    }
    const uint64_t one = ones & ~twos;
    if (!__syncthreads_or(one != 0)) continue;
    const uint64_t pods = a.cls_n[c];
    for (uint32_t x0 = t0; x0 < t1; x0 += EFF_TCH) {
      const uint32_t nt = min(EFF_TCH, t1 - x0);
      for (uint32_t x = 0; x < nt; x++) {
        const uint64_t w = act && one ? eff_allow_word<EG>(a, a.cls_t[x0 + x], kk, j, wl) & one : 0ull;
        const uint64_t s = eff_wave_sum(__popcll(w));
        if (lane == 0) part[wave][x] = s;
      }
      __syncthreads();
      if (threadIdx.x < nt) {
        const uint64_t s = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
        if (s) atomicAdd(&a.sole[uint64_t(a.cls_t[x0 + threadIdx.x]) * a.nk + kk], (unsigned long long)(s * pods));
      }
      __syncthreads();
    }
  }
}

}  // namespace cyc
