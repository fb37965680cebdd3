// dev_closure.hpp — the reflexive transitive closure of a table's adjacency plane and the zones read off it
// (cyc_table_closure, cyc_table_zones).  The reference has no such summary.  Row p of the closure is the row
// cyc_table_reach returns for the seed set {p} with no hop bound: FROM bit q = a path of >= 0 edges p -> q.
//
// The plane C is [P][pitch] with pitch = W rounded up to 16 words: k_table_adjacency's rows, the padding words zeroed
// and the diagonal set (k_closure_start).  No bit at or beyond P is ever set in it.  The closure is a blocked
// bit-Warshall, one pivot word kb = 64 pivots [64 kb, 64 kb + 64) a step, two launches a step:
//   k_closure_panel   every wave closes the diagonal tile D (word kb of the 64 pivot rows: lane = pivot row, 64 steps of
//                     broadcast and OR) into D*, then forms for its 16 column words
//                         panel[i][w] = OR over k in D*[i] of row[k][w]
//                     and writes it to the panel buffer [64][pitch] and back into the pivot rows, word kb excepted: the
//                     other waves of the launch read that word as D.  The blocks behind the panel's copy word kb of
//                     every row into mcol[P].
//   k_closure_update  row i outside the pivots:  row[i][w] |= OR over k in mcol[i] of panel[k][w].  A block owns
//                     CU_ROWS rows and CU_CHUNK column words, stages its chunk of the panel in the LDS and gives a row
//                     to a wave: m = mcol[i] is wave-uniform, a row with m == 0 is left without touching its words, a
//                     lane holds two neighbouring words (16 bytes: of the row in memory, of a panel row in the LDS) and
//                     stores them only where they changed.  Word kb of such a row needs no step of its own:
//                     OR over k in m of D*[k] is what the update computes there.  Word kb of a pivot row is stored here
//                     from the panel (nobody reads it in this launch).
// The mask comes from the snapshot and the panel from its own buffer, so within one launch no word is written by one
// thread and read by another, and every (row, word) has one writer: no atomics, the same bits from run to run.
// A pivot at or beyond P has an empty row and no bit in any mask: it contributes nothing.
//
// k_closure_zones is one transposing pass over the FROM closure in k_table_adjacency's block shape (lane = pod r, 16
// waves on 16 neighbouring row words that walk the column words together): T = transpose64 of word rw of the 64 pods
// of column word cw are the pods of that word that reach r; popc(T) adds up to n_to[r], the lane's own words to
// n_from[r], and the first non-zero T & C[r][cw] holds the smallest pod that r reaches and that reaches r: the
// representative of r's zone (bit r itself is mutual, so rep[r] <= r).  One writer per pod.
#pragma once

namespace cyc {

constexpr uint32_t CP_WORDS = TT_WORDS;  // column words of a wave of the panel: one 128-byte line of each pivot row
constexpr uint32_t CP_WAVES = 4;         // waves of a panel block
constexpr uint32_t CU_CHUNK = 128;       // column words of an update block: 64 x 128 words = 64 KiB of LDS, two blocks a CU
constexpr uint32_t CU_ROWS = 512;        // rows of an update block (the staging is shared by that many rows)
constexpr uint32_t CU_THREADS = 512;     // 8 waves: a row a wave at a time

struct ClosureArgs {
  uint32_t P, W, pitch;  // C: [P][pitch], 16-byte aligned, pitch a multiple of 16
  uint32_t kb;           // the pivot word of the step
  uint32_t panel_blocks; // k_closure_panel: blocks that form the panel; the blocks behind them take the snapshot
  uint64_t* c;
  uint64_t* panel;       // [64][pitch]
  uint64_t* mcol;        // [P]
};

// The start: the padding words of every row zeroed, the diagonal set.  A thread per row (after k_table_adjacency, which
// wrote the words below W).
__global__ __launch_bounds__(256) void k_closure_start(ClosureArgs a) {
  const uint64_t p = blockIdx.x * uint64_t(blockDim.x) + threadIdx.x;
  if (p >= a.P) return;
  uint64_t* row = a.c + p * a.pitch;
  for (uint32_t w = a.W; w < a.pitch; w++) row[w] = 0;
  row[p / 64] |= uint64_t(1) << (p % 64);
}

__device__ __forceinline__ uint64_t lane_word(uint64_t v, uint32_t k) {  // lane k's v in every lane (k wave-uniform)
  const uint32_t lo = __builtin_amdgcn_readlane(uint32_t(v), k), hi = __builtin_amdgcn_readlane(uint32_t(v >> 32), k);
  return uint64_t(hi) << 32 | lo;
}

// lane i holds row i of a reflexive 64 x 64 bit matrix -> row i of its transitive closure (Warshall, pivot k a step)
__device__ __forceinline__ uint64_t close64(uint64_t d) {
#ifndef CYC_DEFECT_CLOSURE_DIAG  // (a planted defect of the tests: the diagonal tile stays as it is)
#pragma unroll 8
  for (uint32_t k = 0; k < 64; k++) {
    const uint64_t dk = lane_word(d, k);
    if (d >> k & 1) d |= dk;
  }
#endif
  return d;
}

__global__ __launch_bounds__(CP_WAVES * 64) void k_closure_panel(ClosureArgs a) {
  if (blockIdx.x >= a.panel_blocks) {  // the snapshot: word kb of every row, a thread per row
    const uint64_t p = (blockIdx.x - a.panel_blocks) * uint64_t(blockDim.x) + threadIdx.x;
    if (p < a.P) a.mcol[p] = a.c[p * a.pitch + a.kb];
    return;
  }
  const uint32_t lane = threadIdx.x & 63, w0 = (blockIdx.x * CP_WAVES + (threadIdx.x >> 6)) * CP_WORDS;
  if (w0 >= a.pitch) return;  // (wave-uniform; pitch is a multiple of CP_WORDS)
  const uint32_t piv = a.kb * 64 + lane;
  const bool p_ok = piv < a.P;
  const uint64_t* row = a.c + uint64_t(piv) * a.pitch;
  // the diagonal tile, closed; a pivot row at or beyond P is empty but for its own bit
  const uint64_t ds = close64((p_ok ? row[a.kb] : 0ull) | uint64_t(1) << lane);
  uint64_t x[CP_WORDS], acc[CP_WORDS];
#pragma unroll
  for (uint32_t j = 0; j < CP_WORDS; j++) x[j] = p_ok ? row[w0 + j] : 0ull, acc[j] = 0;
  for (uint32_t k = 0; k < 64; k++) {
    const bool on = ds >> k & 1;
#pragma unroll
    for (uint32_t j = 0; j < CP_WORDS; j++) {
      const uint64_t v = lane_word(x[j], k);
      if (on) acc[j] |= v;
    }
  }
#pragma unroll
  for (uint32_t j = 0; j < CP_WORDS; j++) {
    a.panel[uint64_t(lane) * a.pitch + w0 + j] = acc[j];
    // (word kb of the pivot rows is the other waves' diagonal tile: k_closure_update stores it)
    if (p_ok && w0 + j != a.kb && acc[j] != x[j]) a.c[uint64_t(piv) * a.pitch + w0 + j] = acc[j];
  }
}

__global__ __launch_bounds__(CU_THREADS) void k_closure_update(ClosureArgs a) {
  __shared__ ulonglong2 pan[64 * CU_CHUNK / 2];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t c0 = blockIdx.x * CU_CHUNK, cn = min(CU_CHUNK, a.pitch - c0);  // (pitch is even: cn too)
  const uint32_t r0 = blockIdx.y * CU_ROWS, r_end = min(r0 + CU_ROWS, a.P);
  const uint32_t piv0 = a.kb * 64;
#ifdef CYC_DEFECT_CLOSURE_SKIP_GROUP  // (a planted defect of the tests: no update when the first row group's masks are empty)
  if (!__syncthreads_or(tid < min(CU_ROWS, a.P) && a.mcol[tid] != 0)) return;
#endif
  // the block's chunk of the panel, 16 bytes a thread (the words at or beyond cn are never read)
  for (uint32_t i = tid; i < 64 * (CU_CHUNK / 2); i += CU_THREADS) {
    const uint32_t k = i / (CU_CHUNK / 2), w = i % (CU_CHUNK / 2) * 2;
    if (w < cn) pan[i] = *reinterpret_cast<const ulonglong2*>(a.panel + uint64_t(k) * a.pitch + c0 + w);
  }
  __syncthreads();
  const uint32_t w = lane * 2;
  const bool in_row = w < cn;
  for (uint32_t r = r0 + wave; r < r_end; r += CU_THREADS / 64) {
    if (r - piv0 < 64) {  // a pivot row: the panel wrote it, word kb excepted
#ifndef CYC_DEFECT_CLOSURE_PIVOT_WORD  // (a planted defect of the tests: word kb of the pivot rows stays the open tile)
      const uint32_t x = a.kb - c0;  // (wraps when the chunk does not hold kb)
      if (x < cn && lane == x / 2) {
        const ulonglong2 v = pan[(r - piv0) * (CU_CHUNK / 2) + lane];
        a.c[uint64_t(r) * a.pitch + a.kb] = x & 1 ? v.y : v.x;
      }
#endif
      continue;
    }
    uint64_t m = uniform64(a.mcol[r]);
    if (!m || !in_row) continue;
    ulonglong2* at = reinterpret_cast<ulonglong2*>(a.c + uint64_t(r) * a.pitch + c0 + w);
    const ulonglong2 old = *at;
    ulonglong2 acc = old;
    do {
      const ulonglong2 v = pan[uint32_t(__builtin_ctzll(m)) * (CU_CHUNK / 2) + lane];
      acc.x |= v.x, acc.y |= v.y;
      m &= m - 1;
    } while (m);
    if (acc.x != old.x) at->x = acc.x;
    if (acc.y != old.y) at->y = acc.y;
  }
}

// n_reach: the set bits of every row.  A wave per row.
__global__ __launch_bounds__(256) void k_closure_counts(ClosureArgs a, unsigned long long* n_reach) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t p = blockIdx.x * uint64_t(blockDim.x / 64) + (threadIdx.x >> 6);
  if (p >= a.P) return;
  uint32_t n = 0;
  for (uint32_t w = lane; w < a.W; w += 64) n += __popcll(a.c[p * a.pitch + w]);
#pragma unroll
  for (int m = 32; m; m >>= 1) n += __shfl_xor(n, m, 64);
  if (lane == 0) n_reach[p] = n;
}

// The plane without its padding: [P][pitch] -> [P][W] (8-byte aligned), a word a thread at a time.
__global__ __launch_bounds__(256) void k_closure_copy(ClosureArgs a, uint64_t* out) {
  const uint64_t n = uint64_t(a.P) * a.W, step = gridDim.x * uint64_t(blockDim.x);
  for (uint64_t i = blockIdx.x * uint64_t(blockDim.x) + threadIdx.x; i < n; i += step) out[i] = a.c[i / a.W * a.pitch + i % a.W];
}

struct ZoneArgs {
  uint32_t P, W, pitch;
  const uint64_t* c;          // the FROM closure
  uint32_t* rep;              // [P]: the smallest pod of the pod's zone
  unsigned long long* n_from; // [P]
  unsigned long long* n_to;   // [P]
};

__global__ __launch_bounds__(1024) void k_closure_zones(ZoneArgs a) {
  const uint32_t lane = threadIdx.x & 63, rw = blockIdx.x * TT_WORDS + (threadIdx.x >> 6);
  // (a wave past the last row word loads nothing and only keeps the block's barriers)
  const uint32_t r = rw * 64 + lane;
  const bool r_ok = rw < a.W && r < a.P;
  uint32_t rep = ~0u, n_from = 0, n_to = 0;
  for (uint32_t cw0 = 0; cw0 < a.W; cw0 += TT_WORDS) {
    // the lane's own words of these columns: one line (the padding words are zero)
    uint64_t ow[TT_WORDS];
#pragma unroll
    for (uint32_t j = 0; j < TT_WORDS; j++) ow[j] = r_ok ? a.c[uint64_t(r) * a.pitch + cw0 + j] : 0ull;
#pragma unroll
    for (uint32_t j = 0; j < TT_WORDS; j++) {
      const uint32_t cw = cw0 + j;
      if (cw >= a.W) continue;
      __syncthreads();  // the block's waves take a tile step together (a line of the column pods' rows: dev_table.hpp)
      // a column pod at or beyond P loads nothing: its bit is 0 in every lane after the transpose
      const bool c_ok = rw < a.W && cw * 64 + lane < a.P;
      const uint64_t t = transpose64(c_ok ? a.c[uint64_t(cw * 64 + lane) * a.pitch + rw] : 0ull, lane);
      n_to += __popcll(t), n_from += __popcll(ow[j]);
      const uint64_t both = t & ow[j];
      if (both && rep == ~0u) rep = cw * 64 + uint32_t(__builtin_ctzll(both));
    }
  }
  if (!r_ok) return;
  a.rep[r] = rep, a.n_from[r] = n_from, a.n_to[r] = n_to;  // (this lane owns the pod)
}

}  // namespace cyc
