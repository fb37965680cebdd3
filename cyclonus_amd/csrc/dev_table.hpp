// dev_table.hpp — whole-table consumers of a device-resident verdict table: connectivity counts
// (the Result / Printer summaries) and the comparison of two tables (connectivity.ComparisonTable,
// pkg/connectivity/comparisontable.go:38-134), computed where the planes are.
//
// Combined(s, d, k) = ingress[d][k][s] AND egress[s][k][d] pairs a bit of a destination-keyed plane
// with a bit of a source-keyed plane.  k_table_tiles gives a wave 64 destinations (lane = d) of one
// 64-pod destination word; per (slot, 64-source word) tile the lanes hold their ingress words as they
// lie in the plane (bits over sources) and bring the matching egress tile (lane = s, bits over d) into
// that orientation with a 64 x 64 bit transpose across the wave.  The per-lane popcounts are the
// per-(d, k) counts; the OR over slots of the compare's XOR is the lane's word of d_diff.
//
// Memory: a block is 16 waves on 16 neighbouring destination words, walking 16 source words together.
// A wave's ingress loads are 8 bytes of 64 rows, and over the 16 source words it consumes those 64
// lines whole: a lane loads its words of several tiles back to back, while its line is in the L1.  The 16
// waves' egress loads of one source word are the 16 words of the same 64 lines, so the waves take each tile
// step together (a barrier per step): left to drift, they spread a line's 16 uses over more traffic than the
// L1 and the XCD's L2 hold, and the line comes from HBM again.  Rows whose length is no multiple of 16 words
// put a 16-word group on two lines, shared with the neighbouring block.  All plane loads are 8-byte loads:
// planes at 8-byte alignment take the same path.
#pragma once

namespace cyc {

// Six-stage butterfly: stage J swaps, between lanes l and l ^ 2^J, the off-diagonal 2^J x 2^J blocks.
__device__ __forceinline__ uint64_t shfl_xor64(uint64_t v, int m) {
  const uint32_t lo = __shfl_xor(uint32_t(v), m, 64), hi = __shfl_xor(uint32_t(v >> 32), m, 64);
  return uint64_t(hi) << 32 | lo;
}
template <int J>
__device__ __forceinline__ uint64_t transpose_stage(uint64_t x, uint32_t lane) {
  constexpr int w = 1 << J;
  constexpr uint64_t m = J == 0 ? 0x5555555555555555ull : J == 1 ? 0x3333333333333333ull : J == 2 ? 0x0F0F0F0F0F0F0F0Full
                       : J == 3 ? 0x00FF00FF00FF00FFull : 0x0000FFFF0000FFFFull;
  const uint64_t y = shfl_xor64(x, w);
  return lane & w ? (x & ~m) | ((y & ~m) >> w) : (x & m) | ((y & m) << w);
}
// lane i holds row i of a 64 x 64 bit matrix (bit j = column j) -> lane j holds column j (bit i = row i)
__device__ __forceinline__ uint64_t transpose64(uint64_t x, uint32_t lane) {
  // stage 5 moves whole halves: lanes 0-31 take their partner's low half, lanes 32-63 its high half
  const bool lower = lane & 32;
  const uint32_t got = __shfl_xor(lower ? uint32_t(x) : uint32_t(x >> 32), 32, 64);
  x = lower ? (x & 0xFFFFFFFF00000000ull) | got : (x & 0xFFFFFFFFull) | uint64_t(got) << 32;
  x = transpose_stage<4>(x, lane);
  x = transpose_stage<3>(x, lane);
  x = transpose_stage<2>(x, lane);
  x = transpose_stage<1>(x, lane);
  return transpose_stage<0>(x, lane);
}

struct TablePlanes {
  const uint64_t *in, *eg;  // layout: include/cyclonus_hip.h (ingress rows over words [w0, w0 + WA))
  const uint8_t* status;    // [P][K]
};

constexpr uint32_t TT_BATCH = 4;   // compare: tiles per batch of ingress loads (two tables' words are held)
constexpr uint32_t TT_WORDS = 16;  // a block's tile: 16 destination words x 16 source words, every slot of the range

struct TileArgs {
  uint32_t P, K, W;
  uint32_t WA, w0;      // ingress window: words [w0, w0 + WA) of every destination's row
  uint32_t s_lo, s_hi;  // the table's sources (s_lo = 64 * w0): egress rows are keyed by s - s_lo
  uint32_t k_lo, nk;
  uint32_t ignore_loopback;
  TablePlanes a, b;  // (counts: only a)
  // Destination-minor, so a wave's 64 atomic adds are 512 contiguous bytes (lanes on 64 different lines add
  // an order of magnitude slower):
  // counts: [nk][3][P] allowed cells of Ingress, Egress, Combined per (k, d)
  // compare: [nk + 2][P]: differing cells per (k, d) (loopback left out when it is ignored), then per d
  //          the differing pairs and whether the pair (d, d) differs
  unsigned long long* cnt;
  uint64_t* diff;  // compare, optional: [P][WA]
};

// bits of word sw that are sources of the table (plane bits at or beyond s_hi are ignored)
__device__ __forceinline__ uint64_t source_mask(uint32_t sw, uint32_t s_hi) {
  const uint32_t base = sw * 64;
  return s_hi >= base + 64 ? ~0ull : s_hi > base ? (1ull << (s_hi - base)) - 1 : 0ull;
}

template <bool CMP>
__global__ __launch_bounds__(1024) void k_table_tiles(TileArgs a) {
  const uint32_t lane = threadIdx.x & 63, dw = blockIdx.x * TT_WORDS + (threadIdx.x >> 6);
  // (a wave past the last destination word loads nothing and only keeps the block's barriers)
  const uint32_t d = dw * 64 + lane;
  const bool d_ok = dw < a.W && d < a.P;
  const uint32_t sw0 = a.w0 + blockIdx.y * TT_WORDS, sw_end = min(sw0 + TT_WORDS, a.w0 + a.WA);
  const uint64_t eg_step = uint64_t(64) * a.K * a.W;
  uint64_t diff[TT_WORDS];
#pragma unroll
  for (uint32_t j = 0; j < TT_WORDS; j++) diff[j] = 0;
  for (uint32_t kk = 0; kk < a.nk; kk++) {
    const uint32_t k = a.k_lo + kk;
    const uint8_t sa = d_ok ? a.a.status[uint64_t(d) * a.K + k] : uint8_t(CYC_JOB_NONE);
    // word j of the block's source words: the lane's ingress word (lane = d), and the egress word dw of
    // source 64 * (sw0 + j) + lane (lane = s), one step of 64 rows further per j
    const uint64_t in_at = (uint64_t(d) * a.K + k) * a.WA + (sw0 - a.w0);
    const uint64_t eg_at = (uint64_t(sw0 * 64 + lane - a.s_lo) * a.K + k) * a.W + dw;
    if (CMP) {
      // cell codes (cyc_table_cells): both VALID -> the Combined bits decide; otherwise the code is a
      // function of the status alone and two different statuses are two different codes
      const uint8_t sb = d_ok ? a.b.status[uint64_t(d) * a.K + k] : uint8_t(CYC_JOB_NONE);
      const bool both = sa == CYC_JOB_VALID && sb == CYC_JOB_VALID, all_differ = !both && sa != sb;
      const bool any_both = __ballot(both) != 0;
      uint64_t n = 0;
#pragma unroll
      for (uint32_t h = 0; h < TT_WORDS; h += TT_BATCH) {
        // the lane's ingress words of TT_BATCH tiles, loaded back to back: they share a line, which is then
        // fetched once per batch instead of once per tile (a block's 1024 ingress lines do not stay in the L1
        // over a tile step)
        uint64_t ia[TT_BATCH], ib[TT_BATCH];
#pragma unroll
        for (uint32_t j = 0; j < TT_BATCH; j++) {
          const bool on = both && sw0 + h + j < sw_end;
          ia[j] = on ? a.a.in[in_at + h + j] : 0ull;
          ib[j] = on ? a.b.in[in_at + h + j] : 0ull;
        }
#pragma unroll
        for (uint32_t j = 0; j < TT_BATCH; j++) {
          const uint32_t sw = sw0 + h + j;
          if (sw >= sw_end) continue;
          __syncthreads();  // the block's waves take a tile step together (its egress lines: header comment)
          uint64_t x = all_differ ? ~0ull : 0ull;
          if (any_both) {
            const bool s_ok = dw < a.W && sw * 64 + lane < a.s_hi;
            const uint64_t ta = transpose64(s_ok ? a.a.eg[eg_at + (h + j) * eg_step] : 0ull, lane);
            const uint64_t tb = transpose64(s_ok ? a.b.eg[eg_at + (h + j) * eg_step] : 0ull, lane);
            if (both) x = (ta & ia[j]) ^ (tb & ib[j]);
          }
          x &= source_mask(sw, a.s_hi);
          diff[h + j] |= x;
          if (a.ignore_loopback && sw == dw) x &= ~(1ull << lane);
          n += __popcll(x);
        }
      }
      if (sa != CYC_JOB_NONE && n) atomicAdd(&a.cnt[uint64_t(kk) * a.P + d], (unsigned long long)n);
    } else {
      const bool valid = sa == CYC_JOB_VALID;
      const bool any_valid = __ballot(valid) != 0;  // (status-only slots need no plane read)
      uint64_t ni = 0, ne = 0, nc = 0;
      uint64_t iw[TT_WORDS];  // the lane's ingress words of the block's tiles: one line, loaded back to back
#pragma unroll
      for (uint32_t j = 0; j < TT_WORDS; j++) iw[j] = valid && sw0 + j < sw_end ? a.a.in[in_at + j] : 0ull;
#pragma unroll
      for (uint32_t j = 0; j < TT_WORDS; j++) {
        const uint32_t sw = sw0 + j;
        if (sw >= sw_end) continue;
        __syncthreads();  // the block's waves take a tile step together (its egress lines: header comment)
        if (!any_valid) continue;
        const uint64_t t = transpose64(sw * 64 + lane < a.s_hi ? a.a.eg[eg_at + j * eg_step] : 0ull, lane);
        if (valid) {
          const uint64_t m = source_mask(sw, a.s_hi), i = iw[j] & m;
          ni += __popcll(i);
          ne += __popcll(t & m);
          nc += __popcll(t & i);
        }
      }
      if (valid) {
        unsigned long long* o = a.cnt + uint64_t(kk) * 3 * a.P + d;
        if (ni) atomicAdd(o, (unsigned long long)ni);
        if (ne) atomicAdd(o + a.P, (unsigned long long)ne);
        if (nc) atomicAdd(o + 2 * uint64_t(a.P), (unsigned long long)nc);
      }
    }
  }
  if (CMP && d_ok) {
    uint64_t pairs = 0;
    bool self = false;
#pragma unroll
    for (uint32_t j = 0; j < TT_WORDS; j++) {
      const uint32_t sw = sw0 + j;
      if (sw >= sw_end) continue;
      if (a.diff) a.diff[uint64_t(d) * a.WA + (sw - a.w0)] = diff[j];  // (this wave owns the word)
      pairs += __popcll(diff[j]);
      if (sw == dw) self = (diff[j] >> lane) & 1;
    }
    unsigned long long* o = a.cnt + uint64_t(a.nk) * a.P + d;
    if (pairs) atomicAdd(o, (unsigned long long)pairs);
    if (self) atomicAdd(o + a.P, 1ull);
  }
}

// ---- A partial target-row table: ingress rows of its destinations, egress rows of its sources.  No
// cell has both, so there is no Combined and no transpose: two row reductions.
struct RowCountArgs {
  uint32_t P, K, W, row_lo, rows, k_lo, nk;
  TablePlanes t;
  uint64_t* valid;          // [nk][W]: bit d of word w = status[d][k] is VALID
  unsigned long long* cnt;  // [rows][nk][2]: allowed Ingress cells of destination row r, allowed Egress cells of source row r
};
__global__ __launch_bounds__(256) void k_table_valid_words(RowCountArgs a) {
  const uint64_t i = blockIdx.x * uint64_t(blockDim.x) + threadIdx.x;
  if (i >= uint64_t(a.nk) * a.W) return;
  const uint32_t kk = uint32_t(i / a.W), w = uint32_t(i % a.W);
  uint64_t m = 0;
  for (uint32_t b = 0; b < 64 && w * 64 + b < a.P; b++)
    if (a.t.status[uint64_t(w * 64 + b) * a.K + a.k_lo + kk] == CYC_JOB_VALID) m |= 1ull << b;
  a.valid[i] = m;
}
// a wave per (row, slot)
__global__ __launch_bounds__(256) void k_table_row_counts(RowCountArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t item = blockIdx.x * uint64_t(blockDim.x / 64) + (threadIdx.x >> 6);
  if (item >= uint64_t(a.rows) * a.nk) return;
  const uint32_t r = uint32_t(item / a.nk), kk = uint32_t(item % a.nk), k = a.k_lo + kk;
  const bool valid = a.t.status[uint64_t(a.row_lo + r) * a.K + k] == CYC_JOB_VALID;
  const uint64_t row = (uint64_t(r) * a.K + k) * a.W;
  uint64_t ni = 0, ne = 0;
  for (uint32_t w = lane; w < a.W; w += 64) {
    if (valid) ni += __popcll(a.t.in[row + w] & source_mask(w, a.P));
    ne += __popcll(a.t.eg[row + w] & a.valid[uint64_t(kk) * a.W + w]);
  }
  for (int m = 32; m; m >>= 1) ni += shfl_xor64(ni, m), ne += shfl_xor64(ne, m);
  if (lane == 0) a.cnt[item * 2] = ni, a.cnt[item * 2 + 1] = ne;
}

}  // namespace cyc
