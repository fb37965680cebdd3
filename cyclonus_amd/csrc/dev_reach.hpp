// dev_reach.hpp — multi-hop reachability over a device-resident verdict table (cyc_table_adjacency, cyc_table_reach).
// The reference has no such summary; an edge is a Combined of allowed (policy.go:123-125) in some slot of the range:
//   s -> d  iff  some k in [k_lo, k_hi) has status[d][k] VALID, ingress[d][k][s] set and egress[s][k][d] set.
// Combined pairs a bit of the destination-keyed plane with a bit of the source-keyed plane (dev_table.hpp), so the
// row "everything s talks to" exists nowhere.  k_table_adjacency materialises it once as a bit plane [P][pitch]:
//   FROM  row s, bit d = edge s -> d.  Lane = source (the orientation of find_words): a wave's own words are the egress
//         words of its row, the ingress tile (lane = d) comes through transpose64, the VALID destinations of a
//         (slot, destination word) are word 0 of k_find_status_words.
//   TO    row d, bit s = edge s -> d, the transpose.  Lane = destination (k_table_tiles' orientation): the own words
//         are the ingress words, the egress tile (lane = s) is transposed, VALID is the lane's own status.
// Either way the block is dev_table.hpp's: 16 waves on 16 neighbouring row words that walk 16 column words together,
// a barrier per tile step (a line of the transposed plane is used by the 16 waves at once), the own words of a slot
// loaded back to back (128 contiguous bytes of the lane's row).  8-byte loads throughout.  A lane keeps the OR over
// the slots of its 16 words and stores them once, contiguously: every (row, word) has exactly one writer, no atomics.
//
// k_reach_step is one hop of breadth-first search for all seed sets together, a push over the adjacency rows: a block
// owns (set j, RS_CHUNK words of the set's bitsets).  It walks the set's frontier, gathers the block's chunk of each
// frontier pod's adjacency row (16 bytes a lane, RS_FLIGHT rows in flight) into an OR in registers, and then is the
// only writer of its words of visited, of the next frontier and of its pods' hop values.  A pod is in a frontier at
// most once per set, so a whole search reads at most the adjacency plane once per set, whatever the number of hops.
#pragma once

namespace cyc {

struct AdjArgs {
  uint32_t P, K, W, k_lo, nk;
  uint32_t pitch;       // words per row of adj (>= W; words at or beyond W are not written)
  TablePlanes t;        // a table that answers every cell: ingress and egress are [P][K][W]
  const uint64_t* stw;  // FROM: k_find_status_words' [nk][W][2], word 0 = the VALID destinations
  uint64_t* adj;
};

template <bool TO>
__global__ __launch_bounds__(1024) void k_table_adjacency(AdjArgs a) {
  // rows: the pods the lanes stand for (TO: destinations, FROM: sources); columns: the pods of the bits
  const uint32_t lane = threadIdx.x & 63, rw = blockIdx.x * TT_WORDS + (threadIdx.x >> 6);
  // (a wave past the last row word loads nothing and only keeps the block's barriers)
  const uint32_t r = rw * 64 + lane;
  const bool r_ok = rw < a.W && r < a.P;
  const uint32_t cw0 = blockIdx.y * TT_WORDS, cw_end = min(cw0 + TT_WORDS, a.W);
  const uint64_t* own = TO ? a.t.in : a.t.eg;
  const uint64_t* other = TO ? a.t.eg : a.t.in;
  const uint64_t other_step = uint64_t(64) * a.K * a.W;
  uint64_t acc[TT_WORDS];
#pragma unroll
  for (uint32_t j = 0; j < TT_WORDS; j++) acc[j] = 0;
  for (uint32_t kk = 0; kk < a.nk; kk++) {
    const uint32_t k = a.k_lo + kk;
    const bool on = r_ok && (!TO || a.t.status[uint64_t(r) * a.K + k] == CYC_JOB_VALID);
    const bool any_on = __ballot(on) != 0;
    // the lane's own words of the block's columns: one line, loaded back to back; word rw of the column pod
    // 64 * (cw0 + j) + lane in the other plane, one step of 64 rows further per j
    const uint64_t own_at = (uint64_t(r) * a.K + k) * a.W + cw0;
    const uint64_t other_at = (uint64_t(cw0 * 64 + lane) * a.K + k) * a.W + rw;
    uint64_t ow[TT_WORDS];
#pragma unroll
    for (uint32_t j = 0; j < TT_WORDS; j++) ow[j] = on && cw0 + j < cw_end ? own[own_at + j] : 0ull;
#pragma unroll
    for (uint32_t j = 0; j < TT_WORDS; j++) {
      const uint32_t cw = cw0 + j;
      if (cw >= cw_end) continue;
      __syncthreads();  // the block's waves take a tile step together (the other plane's lines: dev_table.hpp)
      if (!any_on) continue;
      // FROM: the VALID destinations of the column word (no bit at or beyond P); TO: the lane's status is in `on`
      const uint64_t vw = TO ? ~0ull : uniform64(a.stw[(uint64_t(kk) * a.W + cw) * 2]);
      if (!vw) continue;
      // a column pod at or beyond P loads nothing: its bit is 0 in every lane after the transpose
      const bool c_ok = rw < a.W && cw * 64 + lane < a.P;
      acc[j] |= transpose64(c_ok ? other[other_at + j * other_step] : 0ull, lane) & ow[j] & vw;
    }
  }
  if (!r_ok) return;
#pragma unroll
  for (uint32_t j = 0; j < TT_WORDS; j++)
    if (cw0 + j < cw_end) a.adj[uint64_t(r) * a.pitch + cw0 + j] = acc[j];  // (this lane owns the word)
}

// ---- the search
constexpr uint32_t RS_THREADS = 256;          // a block of the step
constexpr uint32_t RS_CHUNK = 2 * RS_THREADS;  // its words of a set's bitsets: two a thread, one 16-byte load of a row
constexpr uint32_t RS_LIST = 1024;             // frontier pods listed in the LDS at a time
constexpr uint32_t RS_FLIGHT = 8;              // adjacency rows a thread has in flight

struct ReachArgs {
  uint32_t P, W, pitch;  // adj: [P][pitch], pitch even and the plane 16-byte aligned; the bitsets: [n_sets][W]
  uint32_t chunks;       // blocks per set: ceil(W / RS_CHUNK)
  int32_t hop;
  const uint64_t* adj;
  const uint64_t* front;    // pods first reached at hop - 1
  uint64_t* next;           // out: pods first reached at this hop (every word is written)
  uint64_t* visited;        // in/out
  int32_t* hops;            // [n_sets][P] or null: `hop` is stored for the new pods
  unsigned long long* cnt;  // [n_sets], zeroed: new pods of the set
};

__device__ __forceinline__ void reach_store_hops(int32_t* row, uint32_t w, uint64_t bits, int32_t hop) {
  while (bits) {
    row[w * 64 + uint32_t(__builtin_ctzll(bits))] = hop;
    bits &= bits - 1;
  }
}

// hop 0: the seeds.  A thread per (set, word) of the first frontier.
__global__ __launch_bounds__(256) void k_reach_seed_hops(ReachArgs a, uint64_t n_words) {
  const uint64_t i = blockIdx.x * uint64_t(blockDim.x) + threadIdx.x;
  if (i >= n_words) return;
  reach_store_hops(a.hops + (i / a.W) * a.P, uint32_t(i % a.W), a.front[i], 0);
}

__global__ __launch_bounds__(RS_THREADS) void k_reach_step(ReachArgs a) {
  __shared__ uint32_t list[RS_LIST];
  __shared__ uint32_t wave_sum[RS_THREADS / 64];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t j = blockIdx.x / a.chunks, w = (blockIdx.x % a.chunks) * RS_CHUNK + tid * 2;
  const bool in_row = w < a.pitch;  // (pitch is even: word w + 1 is inside the row too)
  const uint64_t* front = a.front + uint64_t(j) * a.W;
  const uint64_t* col = a.adj + w;
  uint64_t acc0 = 0, acc1 = 0;
  // the set's frontier, RS_THREADS words at a time: a word per thread, the block's running sum of the popcounts
  // places every pod in a list, which the block then gathers RS_LIST pods at a time
  for (uint32_t f0 = 0; f0 < a.W; f0 += RS_THREADS) {
    const uint32_t fw = f0 + tid;
    const uint64_t f = fw < a.W ? front[fw] : 0ull;
    const uint32_t n = __popcll(f);
    uint32_t incl = n;
#pragma unroll
    for (uint32_t i = 1; i < 64; i <<= 1) {
      const uint32_t v = __shfl_up(incl, i, 64);
      if (lane >= i) incl += v;
    }
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    uint32_t first = incl - n, total = 0;  // the thread's first place in the list; the pods of these words
#pragma unroll
    for (uint32_t q = 0; q < RS_THREADS / 64; q++) {
      const uint32_t s = wave_sum[q];
      if (q < wave) first += s;
      total += s;
    }
    for (uint32_t lo = 0; lo < total; lo += RS_LIST) {
      if (first < lo + RS_LIST && first + n > lo) {
        uint64_t g = f;
        for (uint32_t at = first; g; at++, g &= g - 1)
          if (at >= lo && at < lo + RS_LIST) list[at - lo] = fw * 64 + uint32_t(__builtin_ctzll(g));
      }
      __syncthreads();
      const uint32_t m = min(total - lo, RS_LIST);
      if (in_row)
        for (uint32_t i = 0; i < m; i += RS_FLIGHT) {
          ulonglong2 v[RS_FLIGHT];
          // (past the end the last pod again: an OR takes a row twice without harm)
#pragma unroll
          for (uint32_t u = 0; u < RS_FLIGHT; u++)
            v[u] = *reinterpret_cast<const ulonglong2*>(col + uint64_t(list[min(i + u, m - 1)]) * a.pitch);
#pragma unroll
          for (uint32_t u = 0; u < RS_FLIGHT; u++) acc0 |= v[u].x, acc1 |= v[u].y;
        }
      __syncthreads();  // (the list and wave_sum are free again)
    }
    if (!total) __syncthreads();  // (wave_sum)
  }
  // the thread's two words: it is their only writer in visited, next and (by pod) hops
  uint32_t found = 0;
  const uint64_t acc[2] = {acc0, acc1};
#pragma unroll
  for (uint32_t x = 0; x < 2; x++) {
    if (w + x >= a.W) continue;  // (words of the row's padding hold nothing defined)
    const uint64_t at = uint64_t(j) * a.W + w + x;
    const uint64_t seen = a.visited[at], fresh = acc[x] & ~seen;
    a.next[at] = fresh;
    if (!fresh) continue;
    a.visited[at] = seen | fresh;
    if (a.hops) reach_store_hops(a.hops + uint64_t(j) * a.P, w + x, fresh, a.hop);
    found += __popcll(fresh);
  }
#pragma unroll
  for (int m = 32; m; m >>= 1) found += __shfl_xor(found, m, 64);
  if (lane == 0 && found) atomicAdd(&a.cnt[j], (unsigned long long)found);
}

}  // namespace cyc
