// dev_classes.hpp — connectivity classes of a device-resident verdict table (cyc_table_classes) and its cells for
// lists of pods (cyc_table_cells_at).  The reference has no such summary: it prints every pod (table.go:58-156).
// Two sources are in one class iff their rows of cell codes are equal, two destinations iff their columns are
// (include/cyclonus_hip.h).  The code of a cell under a non-VALID status depends on (d, k) alone, so it never
// separates sources and the host settles it for destinations (class_terms.hpp); what is left to compare are the
// view's allowed bits under VALID statuses.  For the Ingress and Combined views the row "everything s does" pairs
// bits of a destination-keyed plane with bits of a source-keyed one and exists nowhere, so k_table_view_plane
// materialises it one slot at a time as a bit plane V [P][pitch] (dev_reach.hpp's geometry):
//   FROM  row s, bit d = the cell (s, d, k) is allowed in the view and status[d][k] is VALID    (source classes)
//   TO    row d, bit s = the same cell                                                         (destination classes)
// The rest is plain row work over V, a wave per row with 16-byte loads:
//   k_rows_hash    folds a position-dependent 64-bit hash of every row of the slot's V into h[row]
//   k_rows_verify  compares the rows of listed pods word for word with the rows of their candidate representatives
// The hash only proposes the groups; the verification decides, so the result is exact whatever the hash does.
#pragma once

namespace cyc {

struct ViewPlaneArgs {
  uint32_t P, K, W, k;
  uint32_t pitch;       // words per row of v (>= W; words at or beyond W are not written)
  TablePlanes t;        // a table that answers every cell: ingress and egress are [P][K][W]
  const uint64_t* stw;  // FROM: k_find_status_words' [W][2] of slot k, word 0 = the VALID destinations
  uint64_t* v;
};

// k_table_adjacency's block for one slot and one view: 16 waves on 16 neighbouring row words that walk 16 column
// words together, a barrier per tile step where the transposed plane is read (its lines are used by the 16 waves at
// once), 8-byte loads, every (row, word) stored once by the lane that owns it.  The own plane of an orientation is the
// one whose rows lie along V's rows (TO: ingress, FROM: egress), the other one comes through transpose64.  COMBINED
// takes both, the view of the own plane's direction drops the transposed term, the other view the own term.  The VALID
// mask (TO: the lane's status; FROM: the status word of the column) and the P mask (rows at or beyond P are not
// stored; a column pod at or beyond P loads nothing from the other plane, has no bit in the status word, and is masked
// out of an own ingress word) hold for every view.
template <bool TO, int VIEW>
__global__ __launch_bounds__(1024) void k_table_view_plane(ViewPlaneArgs a) {
  constexpr bool OWN = VIEW != (TO ? CYC_VIEW_EGRESS : CYC_VIEW_INGRESS);
  constexpr bool OTHER = VIEW != (TO ? CYC_VIEW_INGRESS : CYC_VIEW_EGRESS);
  const uint32_t lane = threadIdx.x & 63, rw = blockIdx.x * TT_WORDS + (threadIdx.x >> 6);
  // (a wave past the last row word loads nothing and only keeps the block's barriers)
  const uint32_t r = rw * 64 + lane;
  const bool r_ok = rw < a.W && r < a.P;
  const uint32_t cw0 = blockIdx.y * TT_WORDS, cw_end = min(cw0 + TT_WORDS, a.W);
  const uint64_t* own = TO ? a.t.in : a.t.eg;
  const uint64_t* other = TO ? a.t.eg : a.t.in;
  const uint64_t other_step = uint64_t(64) * a.K * a.W;
  const bool on = r_ok && (!TO || a.t.status[uint64_t(r) * a.K + a.k] == CYC_JOB_VALID);
  const bool any_on = __ballot(on) != 0;
  const uint64_t own_at = (uint64_t(r) * a.K + a.k) * a.W + cw0;
  const uint64_t other_at = (uint64_t(cw0 * 64 + lane) * a.K + a.k) * a.W + rw;
  uint64_t ow[TT_WORDS], acc[TT_WORDS];
#pragma unroll
  for (uint32_t j = 0; j < TT_WORDS; j++) {
    acc[j] = 0;
    // the lane's own words of the block's columns: one line, loaded back to back (TO: bits over sources, cut at P)
    ow[j] = !on || cw0 + j >= cw_end ? 0ull : !OWN ? ~0ull : own[own_at + j] & (TO ? source_mask(cw0 + j, a.P) : ~0ull);
  }
#pragma unroll
  for (uint32_t j = 0; j < TT_WORDS; j++) {
    const uint32_t cw = cw0 + j;
    if (cw >= cw_end) continue;
    if (OTHER) __syncthreads();  // the block's waves take a tile step together (the other plane's lines: dev_table.hpp)
    if (!any_on) continue;
    const uint64_t vw = TO ? ~0ull : uniform64(a.stw[uint64_t(cw) * 2]);
    if (!vw) continue;
    uint64_t x = ow[j] & vw;
    if (OTHER) {
      const bool c_ok = rw < a.W && cw * 64 + lane < a.P;
      x &= transpose64(c_ok ? other[other_at + j * other_step] : 0ull, lane);
    }
    acc[j] = x;
  }
  if (!r_ok) return;
#pragma unroll
  for (uint32_t j = 0; j < TT_WORDS; j++)
    if (cw0 + j < cw_end) a.v[uint64_t(r) * a.pitch + cw0 + j] = acc[j];  // (this lane owns the word)
}

// ---- rows of V
constexpr uint32_t CR_THREADS = 256;  // a block of the row kernels: a wave per row
constexpr uint32_t CR_PASS = 128;     // words of a row a wave takes in one pass: 16 bytes a lane

struct RowsArgs {
  uint32_t P, W, pitch;  // v: [P][pitch], pitch even and the plane 16-byte aligned; words at or beyond W hold nothing defined
  const uint64_t* v;
  uint32_t first;        // hash: the first slot of the range (h starts at 0)
  uint64_t* h;           // hash: [P], in/out
  uint32_t n;            // verify: listed pods
  const uint32_t *pod, *rep;  // verify: [n] a pod and its candidate representative
  uint32_t* bad;         // verify: [n], zeroed before the first slot: the rows differed in some slot
};

// a word's share of its row's hash (mix64: dev_select.hpp's splitmix64 finaliser): position dependent, so two rows
// with the same words in other places differ
__device__ __forceinline__ uint64_t word_hash(uint64_t x, uint32_t w) {
  return mix64(x ^ (uint64_t(w) + 1) * 0x9E3779B97F4A7C15ull);
}
__device__ __forceinline__ ulonglong2 row_words(const uint64_t* row, uint32_t w, uint32_t W) {
  // (w is even and below the even pitch: the 16 bytes lie inside the row; what lies at or beyond W is dropped)
  ulonglong2 x = *reinterpret_cast<const ulonglong2*>(row + w);
  if (w + 1 >= W) x.y = 0;
  return x;
}

// h[row] = mix(h[row], the row's hash in this slot).  The row's hash is a sum of word hashes (integer adds: any order
// gives the same value, and the value repeats from run to run); the fold over the slots depends on their order.
__global__ __launch_bounds__(CR_THREADS) void k_rows_hash(RowsArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t r = blockIdx.x * uint64_t(CR_THREADS / 64) + (threadIdx.x >> 6);
  if (r >= a.P) return;
  const uint64_t* row = a.v + r * a.pitch;
  uint64_t s = 0;
  for (uint32_t w = lane * 2; w < a.W; w += CR_PASS) {
    const ulonglong2 x = row_words(row, w, a.W);
    s += word_hash(x.x, w) + (w + 1 < a.W ? word_hash(x.y, w + 1) : 0ull);
  }
#pragma unroll
  for (int m = 32; m; m >>= 1) s += shfl_xor64(s, m);
  if (lane == 0) a.h[r] = mix64(((a.first ? 0ull : a.h[r]) + 0x9E3779B97F4A7C15ull) ^ s);  // (the row's only writer)
}

// bad[i] |= row pod[i] != row rep[i] in this slot's V.  A wave per listed pod; bad[i] has no other writer.
__global__ __launch_bounds__(CR_THREADS) void k_rows_verify(RowsArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t i = blockIdx.x * uint64_t(CR_THREADS / 64) + (threadIdx.x >> 6);
  if (i >= a.n) return;
  const uint64_t* p = a.v + uint64_t(a.pod[i]) * a.pitch;
  const uint64_t* q = a.v + uint64_t(a.rep[i]) * a.pitch;
  bool differ = false;
  for (uint32_t w = lane * 2; w < a.W; w += CR_PASS) {
    const ulonglong2 x = row_words(p, w, a.W), y = row_words(q, w, a.W);
    differ |= x.x != y.x || x.y != y.y;
  }
  if (__ballot(differ) != 0 && lane == 0) a.bad[i] = 1;
}

// ---- k_table_cells (dev_query.hpp) for lists of pods: cell i is (srcs[i / nk / n_d], dsts[i / nk % n_d], k_lo + i % nk)
struct CellsAtArgs {
  CellArgs c;  // (s_lo, d_lo are not used; nd = the destinations listed)
  const int32_t *srcs, *dsts;
};
__global__ __launch_bounds__(256) void k_table_cells_at(CellsAtArgs b) {
  const CellArgs& a = b.c;
  for (uint64_t i = blockIdx.x * uint64_t(blockDim.x) + threadIdx.x; i < a.n; i += uint64_t(gridDim.x) * blockDim.x) {
    const uint32_t k = a.k_lo + uint32_t(i % a.nk);
    const uint64_t sd = i / a.nk;
    const uint32_t d = uint32_t(b.dsts[sd % a.nd]), s = uint32_t(b.srcs[sd / a.nd]);
    const uint8_t st = a.status[uint64_t(d) * a.K + k];
    uint8_t ci = CYC_CONN_NO_JOB, ce = CYC_CONN_NO_JOB, cc = CYC_CONN_NO_JOB;
    if (st == CYC_JOB_VALID) {
      // the host checked that the requested planes cover the listed rows
      const uint64_t iw = a.src ? (uint64_t(d) * a.K + k) * a.WA + (s / 64 - a.w0) : (uint64_t(d - a.row_lo) * a.K + k) * a.W + s / 64;
      const bool ai = a.o_in || a.o_comb ? (a.in[iw] >> (s % 64)) & 1 : false;
      const bool ae = a.o_eg || a.o_comb ? (a.eg[(uint64_t(s - a.row_lo) * a.K + k) * a.W + d / 64] >> (d % 64)) & 1 : false;
      ci = ai ? CYC_CONN_ALLOWED : CYC_CONN_BLOCKED;
      ce = ae ? CYC_CONN_ALLOWED : CYC_CONN_BLOCKED;
      cc = ai && ae ? CYC_CONN_ALLOWED : CYC_CONN_BLOCKED;
    } else if (st == CYC_JOB_BAD_PORT_PROTOCOL) {
      ci = cc = CYC_CONN_INVALID_PORT_PROTOCOL;
      ce = CYC_CONN_UNKNOWN;
    } else if (st == CYC_JOB_BAD_NAMED_PORT) {
      ci = cc = CYC_CONN_INVALID_NAMED_PORT;
      ce = CYC_CONN_UNKNOWN;
    }
    if (a.o_in) a.o_in[i] = ci;
    if (a.o_eg) a.o_eg[i] = ce;
    if (a.o_comb) a.o_comb[i] = cc;
  }
}

}  // namespace cyc
