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
  // The SRC instantiations (cyc_table_pod_counts, cyc_table_pod_compare) also count per source.  Source-minor for
  // the same reason, source 64 * (w0 + j) + lane at [j * 64 + lane]:
  // counts: [nk][WA * 64] allowed cells of `view` per (k, s)
  // compare: [nk + 1][WA * 64]: differing cells per (k, s) where a holds a job (loopback left out when it is
  //          ignored), then per s the differing pairs (whether (s, s) differs is cnt's entry of d = s)
  unsigned long long* src_cnt;
  uint32_t view;  // counts, SRC: cyc_view
};

// bits of word sw that are sources of the table (plane bits at or beyond s_hi are ignored)
__device__ __forceinline__ uint64_t source_mask(uint32_t sw, uint32_t s_hi) {
  const uint32_t base = sw * 64;
  return s_hi >= base + 64 ? ~0ull : s_hi > base ? (1ull << (s_hi - base)) - 1 : 0ull;
}

// Source words of a block's tile (the grid's y step): TT_WORDS, but half as many for the compare with SRC.
constexpr uint32_t tile_source_words(bool cmp, bool src) { return cmp && src ? TT_WORDS / 2 : TT_WORDS; }

// SRC: the mirrored accumulation.  A tile's bits over (s, d) are summed over d per source: for the words the lanes
// hold by destination (the ingress word, the compare's XOR word) that is one more transpose64 and a popcount with
// lane = s; the raw egress word already lies that way.  The block's 16 waves hold 16 destination words of the same
// 64 sources, so they first add into a u32 LDS table [source words][64] (lane-contiguous: no bank conflict; a
// block's sum per source and slot is at most 1024) and once per slot wave j adds word j's 64 sums to the global
// buffer: one 64-bit atomic per (block, slot, source), 512 contiguous bytes a wave.  Integer adds: the results are
// exact and the same from run to run.  The non-SRC instantiations compile to the code they had before SRC existed.
template <bool CMP, bool SRC = false>
__global__ __launch_bounds__(1024) void k_table_tiles(TileArgs a) {
  // the block's source words: the compare holds 16 OR words, two tables' ingress words and two transposes in
  // flight, and with the third transpose it spills at 16
  constexpr uint32_t SW = tile_source_words(CMP, SRC);
  __shared__ uint32_t src_acc[SRC ? TT_WORDS * 64 : 1];  // (a cell per thread: those of words past SW stay 0)
  const uint32_t lane = threadIdx.x & 63, dw = blockIdx.x * TT_WORDS + (threadIdx.x >> 6);
  // (a wave past the last destination word loads nothing and only keeps the block's barriers)
  const uint32_t d = dw * 64 + lane;
  const bool d_ok = dw < a.W && d < a.P;
  const uint32_t sw0 = a.w0 + blockIdx.y * SW, sw_end = min(sw0 + SW, a.w0 + a.WA);
  const uint64_t eg_step = uint64_t(64) * a.K * a.W;
  uint64_t diff[SW];
#pragma unroll
  for (uint32_t j = 0; j < SW; j++) diff[j] = 0;
  if (SRC) src_acc[threadIdx.x] = 0;  // (the first tile step's barrier stands between this and the adds)
  // SRC, the end of a slot: the thread takes its cell of the table (wave j: source word sw0 + j) to slot `slot` of the
  // buffer and clears it; the next tile step's barrier stands between that and the next adds.
  auto drain_src = [&](uint32_t slot) {
    __syncthreads();
    const uint32_t n = src_acc[threadIdx.x], sw = sw0 + (threadIdx.x >> 6);
    if (!n || sw >= sw_end) return;
    src_acc[threadIdx.x] = 0;
    atomicAdd(&a.src_cnt[(uint64_t(slot) * a.WA + (sw - a.w0)) * 64 + lane], (unsigned long long)n);
  };
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
      for (uint32_t h = 0; h < SW; h += TT_BATCH) {
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
          if (SRC) {
            if (sa == CYC_JOB_NONE) x = 0;  // (per job: only cells where a holds one)
            if (__ballot(x != 0) == 0) continue;
            const uint32_t p = __popcll(transpose64(x, lane));
            if (p) atomicAdd(&src_acc[(h + j) * 64 + lane], p);
          }
        }
      }
      if (sa != CYC_JOB_NONE && n) atomicAdd(&a.cnt[uint64_t(kk) * a.P + d], (unsigned long long)n);
    } else {
      const bool valid = sa == CYC_JOB_VALID;
      const uint64_t vmask = __ballot(valid);  // the VALID destinations of the wave's word
      const bool any_valid = vmask != 0;       // (status-only slots need no plane read)
      uint64_t ni = 0, ne = 0, nc = 0;
      uint64_t iw[SW];  // the lane's ingress words of the block's tiles: one line, loaded back to back
#pragma unroll
      for (uint32_t j = 0; j < SW; j++) iw[j] = valid && sw0 + j < sw_end ? a.a.in[in_at + j] : 0ull;
#pragma unroll
      for (uint32_t j = 0; j < SW; j++) {
        const uint32_t sw = sw0 + j;
        if (sw >= sw_end) continue;
        __syncthreads();  // the block's waves take a tile step together (its egress lines: header comment)
        if (!any_valid) continue;
        const uint64_t e = sw * 64 + lane < a.s_hi ? a.a.eg[eg_at + j * eg_step] : 0ull;
        const uint64_t t = transpose64(e, lane);
        if (valid) {
          const uint64_t m = source_mask(sw, a.s_hi), i = iw[j] & m;
          ni += __popcll(i);
          ne += __popcll(t & m);
          nc += __popcll(t & i);
        }
        if (SRC) {
          // lane = s: e is 0 at or beyond s_hi, and so are those lanes of the transposed ingress words (masked above
          // by source bit); iw is 0 in lanes that are not VALID, which leaves the bits of VALID d < P
          const uint32_t p = a.view == CYC_VIEW_EGRESS ? __popcll(e & vmask)
                                                       : __popcll(transpose64(iw[j] & source_mask(sw, a.s_hi), lane) &
                                                                  (a.view == CYC_VIEW_INGRESS ? ~0ull : e));
          if (p) atomicAdd(&src_acc[j * 64 + lane], p);
        }
      }
      if (valid) {
        unsigned long long* o = a.cnt + uint64_t(kk) * 3 * a.P + d;
        if (ni) atomicAdd(o, (unsigned long long)ni);
        if (ne) atomicAdd(o + a.P, (unsigned long long)ne);
        if (nc) atomicAdd(o + 2 * uint64_t(a.P), (unsigned long long)nc);
      }
    }
    if (SRC) drain_src(kk);
  }
  if (CMP && SRC) {
    // the pairs per source: the transposed OR words (lanes that are no destination hold zeros)
    __syncthreads();  // (the last slot's drain cleared the table)
#pragma unroll
    for (uint32_t j = 0; j < SW; j++) {
      if (sw0 + j >= sw_end || __ballot(diff[j] != 0) == 0) continue;
      const uint32_t p = __popcll(transpose64(diff[j], lane));
      if (p) atomicAdd(&src_acc[j * 64 + lane], p);
    }
    drain_src(a.nk);
  }
  if (CMP && d_ok) {
    uint64_t pairs = 0;
    bool self = false;
#pragma unroll
    for (uint32_t j = 0; j < SW; j++) {
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

// ---- The same pass split by pod group pair (cyc_table_group_counts, cyc_table_group_compare): which groups
// (namespaces, say) reach which, and between which the two tables disagree.  The geometry is k_table_tiles';
// what changes is where the popcounts go.  The host hands over, per 64-pod source word, the (group, 64-bit
// mask) entries of the groups present in it, in pod order, so a group that runs over a word boundary is the
// last entry of one word and the first of the next.  A block first copies the entries of its 16 source words
// (1024 at most) to the LDS: read from global memory in the loop, every entry would be a dependent load that
// the whole wave waits for.  Per tile step the wave walks the entries of its source word (the same for every
// lane: LDS broadcast reads); the lane adds popc(word & mask) to a running sum per view, which it keeps while
// consecutive entries carry the same source group.  On a change of source group the wave sums over its
// runs of lanes with one destination group (a segmented scan: the three views' sums travel packed in one
// 64-bit word) and the last lane of each run adds the sum into the block's LDS table, a packed 64-bit cell per
// (source group, destination group) of the block; per slot the block adds the non-zero cells to the global
// buffer.  The block-local dense numbers of the groups come from the host with the entries (it walks the pods
// once anyway), so the kernel needs no numbering preamble.  A block with more than GT_CAP groups among its 1024
// sources or its 1024 destinations adds the runs' sums straight to the global buffer instead.  Integer sums:
// the result does not depend on the path or the order.
constexpr uint32_t GT_CAP = 32;   // LDS table: GT_CAP source groups x GT_CAP destination groups of the block
constexpr uint32_t GT_BITS = 21;  // a block tile holds at most 2^20 cells of a group pair per slot and view
static_assert(GT_CAP * GT_CAP == 1024, "a thread of the block per LDS cell");

struct GroupArgs {
  TileArgs t;  // cnt: counts [nk][3][G][G] allowed cells of Ingress, Egress, Combined per (k, gs, gd), destination-
               // group-minor; compare [nk + 1][G][G]: differing cells per (k, gs, gd) (loopback left out when it is
               // ignored), then the differing pairs; then [G]: the differing pairs (d, d) per group
  uint32_t G;
  const uint32_t* ent_ptr;   // [WA + 1]: the entries of window word j are [ent_ptr[j], ent_ptr[j + 1])
  const uint64_t* ent_mask;  // [E] the sources of the word that are in the group (and in the table's rows)
  const uint32_t* ent_grp;   // [E] the group
  const uint32_t* ent_loc;   // [E] its number among the groups of the block's 16 source words
  const uint32_t* row_ptr;   // [grid.y + 1] -> row_grp: the groups of a block's sources by that number
  const uint32_t* row_grp;
  const int32_t* dst_grp;    // [P] group_of
  const uint32_t* dst_loc;   // [P] the group's number among the groups of the block's 1024 destinations
  const uint32_t* col_ptr;   // [grid.x + 1] -> col_grp
  const uint32_t* col_grp;
};

template <bool CMP>
__global__ __launch_bounds__(1024) void k_table_group_tiles(GroupArgs g) {
  constexpr uint32_t V = CMP ? 1 : 3;
  constexpr uint64_t FIELD = (1ull << GT_BITS) - 1;
  __shared__ unsigned long long tab[GT_CAP * GT_CAP];
  __shared__ uint64_t ent_mask[TT_WORDS * 64];  // the block's entries: mask, and group or its block-local number
  __shared__ uint32_t ent_key[TT_WORDS * 64], ent_at[TT_WORDS + 1];
  const TileArgs& a = g.t;
  const uint32_t lane = threadIdx.x & 63, dw = blockIdx.x * TT_WORDS + (threadIdx.x >> 6);
  // (a wave past the last destination word loads nothing and only keeps the block's barriers)
  const uint32_t d = dw * 64 + lane;
  const int32_t gd = dw < a.W && d < a.P ? g.dst_grp[d] : -1;
  const bool d_ok = gd >= 0;  // (a pod without a group is no destination: its lane holds zeros throughout)
  const uint32_t ld = d_ok ? g.dst_loc[d] : 0;
  const uint32_t sw0 = a.w0 + blockIdx.y * TT_WORDS, sw_end = min(sw0 + TT_WORDS, a.w0 + a.WA);
  const uint64_t eg_step = uint64_t(64) * a.K * a.W, GG = uint64_t(g.G) * g.G;
  const uint32_t rs = g.row_ptr[blockIdx.y], cs = g.col_ptr[blockIdx.x];
  const bool use_lds = g.row_ptr[blockIdx.y + 1] - rs <= GT_CAP && g.col_ptr[blockIdx.x + 1] - cs <= GT_CAP;
  {
    const uint32_t e0 = g.ent_ptr[sw0 - a.w0], n_ent = g.ent_ptr[sw_end - a.w0] - e0;
    if (threadIdx.x <= sw_end - sw0) ent_at[threadIdx.x] = g.ent_ptr[sw0 - a.w0 + threadIdx.x] - e0;
    if (threadIdx.x < n_ent) {
      ent_mask[threadIdx.x] = g.ent_mask[e0 + threadIdx.x];
      ent_key[threadIdx.x] = (use_lds ? g.ent_loc : g.ent_grp)[e0 + threadIdx.x];
    }
  }
  // the wave's runs of lanes with one destination group: the first lane of the lane's run, and whether it is the last
  // (the shuffle stands before the condition: behind `lane == 0 ||` lane 0 would sit it out and lane 1 read a zero)
  const int32_t gd_before = __shfl_up(gd, 1, 64);
  const uint64_t heads = __ballot(lane == 0 || gd != gd_before);
  const uint32_t run_start = 63 - __clzll((long long)(heads & (~0ull >> (63 - lane))));
  const bool tail = lane == 63 || ((heads >> (lane + 1)) & 1);
  tab[threadIdx.x] = 0;
  __syncthreads();

  uint32_t cur = ~0u, n[V];  // the source group of the running sums (its block-local number on the LDS path)
#pragma unroll
  for (uint32_t v = 0; v < V; v++) n[v] = 0;
  // The running sums go to slot `slot` of the buffer.  Wave-uniform: every lane of the wave calls it together.
  auto flush = [&](uint32_t slot) {
    uint64_t s = n[0];
    if (!CMP) s |= uint64_t(n[1]) << GT_BITS | uint64_t(n[2]) << (2 * GT_BITS);
#pragma unroll
    for (uint32_t v = 0; v < V; v++) n[v] = 0;
    if (cur == ~0u || __ballot(s != 0) == 0) return;
    // a lane's sum is at most 1024 per view and a run's at most 2^16: the fields do not carry into each other
#pragma unroll
    for (uint32_t i = 1; i < 64; i <<= 1) {
      const uint32_t lo = __shfl_up(uint32_t(s), i, 64), hi = __shfl_up(uint32_t(s >> 32), i, 64);
      if (lane >= run_start + i) s += uint64_t(hi) << 32 | lo;
    }
    if (!tail || !d_ok || !s) return;
    if (use_lds) {
      atomicAdd(&tab[cur * GT_CAP + ld], (unsigned long long)s);
    } else {
      unsigned long long* o = a.cnt + uint64_t(slot) * V * GG + uint64_t(cur) * g.G + uint32_t(gd);
#pragma unroll
      for (uint32_t v = 0; v < V; v++) {
        const uint64_t c = (s >> (v * GT_BITS)) & FIELD;
        if (c) atomicAdd(o + v * GG, (unsigned long long)c);
      }
    }
  };
  // the words of a tile step (bits over the sources of word sw), split by the source groups of the word
  auto add_word = [&](uint32_t sw, uint64_t x0, uint64_t x1, uint64_t x2, uint32_t slot) {
    const uint32_t e_end = __builtin_amdgcn_readfirstlane(ent_at[sw - sw0 + 1]);
    for (uint32_t e = __builtin_amdgcn_readfirstlane(ent_at[sw - sw0]); e < e_end; e++) {
      const uint32_t key = __builtin_amdgcn_readfirstlane(ent_key[e]);
      if (key != cur) {
        flush(slot);
        cur = key;
      }
      const uint64_t m = ent_mask[e];
      n[0] += __popcll(x0 & m);
      if (!CMP) n[1] += __popcll(x1 & m), n[2] += __popcll(x2 & m);
    }
  };
  // the end of a slot: the last running sums, then the block's LDS cells go to the global buffer
  auto drain = [&](uint32_t slot) {
    flush(slot);
    cur = ~0u;
    if (!use_lds) return;
    __syncthreads();
    const unsigned long long s = tab[threadIdx.x];
    if (s) {
      tab[threadIdx.x] = 0;
      unsigned long long* o = a.cnt + uint64_t(slot) * V * GG + uint64_t(g.row_grp[rs + threadIdx.x / GT_CAP]) * g.G +
                              g.col_grp[cs + threadIdx.x % GT_CAP];
#pragma unroll
      for (uint32_t v = 0; v < V; v++) {
        const uint64_t c = (s >> (v * GT_BITS)) & FIELD;
        if (c) atomicAdd(o + v * GG, (unsigned long long)c);
      }
    }
    __syncthreads();
  };

  uint64_t diff[CMP ? TT_WORDS : 1];
#pragma unroll
  for (uint32_t j = 0; j < (CMP ? TT_WORDS : 1); j++) diff[j] = 0;
  for (uint32_t kk = 0; kk < a.nk; kk++) {
    const uint32_t k = a.k_lo + kk;
    const uint8_t sa = d_ok ? a.a.status[uint64_t(d) * a.K + k] : uint8_t(CYC_JOB_NONE);
    const uint8_t sb = CMP && d_ok ? a.b.status[uint64_t(d) * a.K + k] : uint8_t(CYC_JOB_NONE);
    // counts: the lane's cells are VALID; compare: both are (k_table_tiles: otherwise the statuses decide)
    const bool on = CMP ? sa == CYC_JOB_VALID && sb == CYC_JOB_VALID : sa == CYC_JOB_VALID;
    const bool all_differ = CMP && !on && sa != sb;
    const bool any_on = __ballot(on) != 0, any_word = any_on || __ballot(all_differ) != 0;
    const uint64_t in_at = (uint64_t(d) * a.K + k) * a.WA + (sw0 - a.w0);
    const uint64_t eg_at = (uint64_t(sw0 * 64 + lane - a.s_lo) * a.K + k) * a.W + dw;
#pragma unroll 1
    for (uint32_t h = 0; h < TT_WORDS; h += TT_BATCH) {
      // the lane's ingress words of TT_BATCH tiles, loaded back to back (k_table_tiles)
      uint64_t ia[TT_BATCH], ib[TT_BATCH];
#pragma unroll
      for (uint32_t j = 0; j < TT_BATCH; j++) {
        const bool ld_on = on && sw0 + h + j < sw_end;
        ia[j] = ld_on ? a.a.in[in_at + h + j] : 0ull;
        ib[j] = CMP && ld_on ? a.b.in[in_at + h + j] : 0ull;
      }
#pragma unroll
      for (uint32_t j = 0; j < TT_BATCH; j++) {
        const uint32_t sw = sw0 + h + j;
        if (sw >= sw_end) continue;
        __syncthreads();  // the block's waves take a tile step together (its egress lines: header comment)
        if (!any_word) continue;
        const uint64_t m = source_mask(sw, a.s_hi);
        uint64_t ta = 0, tb = 0;
        if (any_on) {
          const bool s_ok = dw < a.W && sw * 64 + lane < a.s_hi;
          ta = transpose64(s_ok ? a.a.eg[eg_at + (h + j) * eg_step] : 0ull, lane);
          if (CMP) tb = transpose64(s_ok ? a.b.eg[eg_at + (h + j) * eg_step] : 0ull, lane);
        }
        if (CMP) {
          uint64_t x = (on ? (ta & ia[j]) ^ (tb & ib[j]) : all_differ ? ~0ull : 0ull) & m;
          // (h is not unrolled: a select per batch keeps diff[] in registers)
#pragma unroll
          for (uint32_t hh = 0; hh < (CMP ? TT_WORDS : 1); hh += TT_BATCH) diff[hh + (CMP ? j : 0)] |= h == hh ? x : 0ull;
          if (a.ignore_loopback && sw == dw) x &= ~(1ull << lane);
          add_word(sw, sa != CYC_JOB_NONE ? x : 0ull, 0, 0, kk);  // (per job: only cells where a holds one)
        } else {
          const uint64_t i = on ? ia[j] & m : 0ull, e = on ? ta & m : 0ull;
          add_word(sw, i, e, e & i, kk);
        }
      }
    }
    drain(kk);
  }
  if (CMP) {
    // the pairs: the lane's OR over the slots, split by the same entries, as slot nk of the buffer
#pragma unroll 1
    for (uint32_t j = 0; sw0 + j < sw_end; j++) {
      uint64_t x = 0;
#pragma unroll
      for (uint32_t jj = 0; jj < (CMP ? TT_WORDS : 1); jj++) x = j == jj ? diff[jj] : x;
      add_word(sw0 + j, x, 0, 0, a.nk);
      if (sw0 + j == dw && ((x >> lane) & 1)) atomicAdd(a.cnt + (uint64_t(a.nk) + 1) * GG + uint32_t(gd), 1ull);
    }
    drain(a.nk);
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

// ---- Which cells: the listing behind a count (cyc_table_find, cyc_table_compare_find).  The records come in
// (s, d, k) order, source-major like the reference's jobs (resources.go:284-364), so these kernels are the
// mirror image of k_table_tiles: lane = source.  A wave holds 64 sources of one source word; its own words are
// the egress words of its row (bits over d, contiguous in the row) and the ingress tile (lane = d, bits over s)
// comes into that orientation through transpose64.  The status takes part as two bit words over destinations per
// (slot, destination word), built once by k_find_status_words:
//   find:     word 0 = VALID, word 1 = the status-only code of the view is in the mask
//   compare:  word 0 = both VALID, word 1 = a holds a job and the statuses differ
// so a lane's match word is  word1 | word0 & f(ingress bits, egress bits).
// Pass 1 (k_table_find_count) counts the matches per (source, block of 16 destination words): every block of
// the grid owns its counts, plain stores.  k_table_find_scan turns a source's counts into their running sums
// over the destination blocks and its total; the host's prefix sum over the totals places every source's records
// and chooses the page.  Pass 2 (k_table_find_emit) is a wave per (source word of the page, destination block that
// holds a match): a lane starts at its source's place plus the running sum of the block and counts on in a
// register.  No atomics anywhere, so the order is exact by construction.  Both passes take their match words from
// find_words, so they cannot disagree about a cell.
struct FindArgs {
  TileArgs t;                // (cnt: [n_src] matching cells per source)
  uint32_t view, code_mask;  // find
  uint32_t bx0;              // pass 1: the first block of 16 source words (sources before s_from are not asked for)
  uint32_t NB;               // blocks of 16 destination words
  uint64_t* stw;             // [nk][W][2] status words
  uint32_t n_src;            // s_hi - s_lo
  // [NB][n_src], source-minor (a wave's 512 contiguous bytes): pass 1 the matches of (block, source); after the
  // scan those of the source's earlier blocks
  unsigned long long* blk;
  uint32_t s_from, s_next;   // pass 2: the page's sources
  const unsigned long long* offs;  // [s_next - s_from + 1] first record of each source of the page, and the end
  uint4* out;                // the page's records (cyc_cell)
  uint64_t* scratch;         // [grid][nk][4][64] match and code words when they do not fit the LDS, else null
};

template <bool CMP>
__global__ __launch_bounds__(256) void k_find_status_words(FindArgs a) {
  const TileArgs& t = a.t;
  const uint64_t i = blockIdx.x * uint64_t(blockDim.x) + threadIdx.x;
  if (i >= uint64_t(t.nk) * t.W) return;
  const uint32_t k = t.k_lo + uint32_t(i / t.W), w = uint32_t(i % t.W);
  uint64_t x = 0, y = 0;
  for (uint32_t b = 0; b < 64 && w * 64 + b < t.P; b++) {
    const uint8_t sa = t.a.status[uint64_t(w * 64 + b) * t.K + k];
    if (CMP) {
      const uint8_t sb = t.b.status[uint64_t(w * 64 + b) * t.K + k];
      if (sa == CYC_JOB_VALID && sb == CYC_JOB_VALID) x |= 1ull << b;
      else if (sa != CYC_JOB_NONE && sa != sb) y |= 1ull << b;
    } else if (sa == CYC_JOB_VALID) {
      x |= 1ull << b;
    } else if (sa != CYC_JOB_NONE) {
      const uint32_t code = a.view == CYC_VIEW_EGRESS          ? CYC_CONN_UNKNOWN
                            : sa == CYC_JOB_BAD_PORT_PROTOCOL ? CYC_CONN_INVALID_PORT_PROTOCOL
                                                              : CYC_CONN_INVALID_NAMED_PORT;
      if ((a.code_mask >> code) & 1) y |= 1ull << b;
    }
  }
  a.stw[i * 2] = x, a.stw[i * 2 + 1] = y;
}

__device__ __forceinline__ uint64_t uniform64(uint64_t v) {
  return uint64_t(uint32_t(__builtin_amdgcn_readfirstlane(int(uint32_t(v >> 32))))) << 32 |
         uint32_t(__builtin_amdgcn_readfirstlane(int(uint32_t(v))));
}

// Lane = source 64 * sw + lane, bits over the destinations of word dw, slot k_lo + kk: the match word m, the
// ingress and egress words of a (i, e) and b's Combined word (o).  ea, eb are the lane's egress words.  Called
// by whole waves with kk, sw (inside the window) and dw the same in every lane.  ALL: every word is wanted (the
// records carry every code); otherwise only what m needs is loaded.
struct FindWords {
  uint64_t m, i, e, o;
};
template <bool CMP, bool ALL>
__device__ __forceinline__ FindWords find_words(const FindArgs& a, uint32_t kk, uint32_t sw, uint32_t dw, uint32_t lane, bool s_ok,
                                                uint64_t ea, uint64_t eb) {
  const TileArgs& t = a.t;
  const uint64_t* st = a.stw + (uint64_t(kk) * t.W + dw) * 2;
  const uint64_t w0 = uniform64(st[0]), w1 = uniform64(st[1]);
  FindWords f{w1, 0, ea, 0};
  if (ALL || w0) {
    const uint32_t d = dw * 64 + lane;  // (the ingress loads have lane = d)
    const bool d_ok = d < t.P;
    const uint64_t at = (uint64_t(d) * t.K + t.k_lo + kk) * t.WA + (sw - t.w0);
    if (ALL || CMP || a.view != CYC_VIEW_EGRESS) f.i = transpose64(d_ok ? t.a.in[at] : 0ull, lane);
    if (CMP) {
      f.o = transpose64(d_ok ? t.b.in[at] : 0ull, lane) & eb;
      f.m |= w0 & ((f.i & ea) ^ f.o);
    } else {
      const uint64_t x = a.view == CYC_VIEW_INGRESS ? f.i : a.view == CYC_VIEW_EGRESS ? ea : f.i & ea;
      f.m |= w0 & (((a.code_mask >> CYC_CONN_ALLOWED) & 1 ? x : 0ull) | ((a.code_mask >> CYC_CONN_BLOCKED) & 1 ? ~x : 0ull));
    }
  }
  if (CMP && t.ignore_loopback && sw == dw) f.m &= ~(1ull << lane);
  if (!s_ok) f.m = 0;
  return f;
}

// Pass 1.  A block is 16 waves on 16 neighbouring source words, walking 16 destination words together: a lane's
// egress words of the block are 128 contiguous bytes of its row, loaded back to back, and the 16 waves' ingress
// loads of one destination word are the 16 words of the same 64 lines (hence the barrier per step, as in
// k_table_tiles).  The per-lane sums are the block's own: one store per lane, a wave's 512 contiguous bytes.
template <bool CMP>
__global__ __launch_bounds__(1024) void k_table_find_count(FindArgs a) {
  constexpr uint32_t BATCH = CMP ? TT_BATCH : TT_WORDS;  // (compare holds two tables' words)
  const TileArgs& t = a.t;
  const uint32_t lane = threadIdx.x & 63, sw = t.w0 + (a.bx0 + blockIdx.x) * TT_WORDS + (threadIdx.x >> 6);
  // (a wave past the last source word loads nothing and only keeps the block's barriers)
  const bool w_ok = sw < t.w0 + t.WA;
  const uint32_t s = sw * 64 + lane;  // (s >= s_lo = 64 * w0)
  const bool s_ok = w_ok && s < t.s_hi;
  const uint32_t dw0 = blockIdx.y * TT_WORDS, dw_end = min(dw0 + TT_WORDS, t.W);
  uint64_t n = 0;
  for (uint32_t kk = 0; kk < t.nk; kk++) {
    const uint64_t eg_at = (uint64_t(s - t.s_lo) * t.K + t.k_lo + kk) * t.W + dw0;
#pragma unroll 1
    for (uint32_t h = 0; h < TT_WORDS; h += BATCH) {  // (find: one batch)
      uint64_t ea[BATCH], eb[BATCH];
#pragma unroll
      for (uint32_t j = 0; j < BATCH; j++) {
        const bool on = s_ok && dw0 + h + j < dw_end;
        ea[j] = on ? t.a.eg[eg_at + h + j] : 0ull;
        eb[j] = CMP && on ? t.b.eg[eg_at + h + j] : 0ull;
      }
#pragma unroll
      for (uint32_t j = 0; j < BATCH; j++) {
        const uint32_t dw = dw0 + h + j;
        if (dw >= dw_end) continue;
        __syncthreads();  // the block's waves take a step together (its ingress lines)
        if (w_ok) n += __popcll(find_words<CMP, false>(a, kk, sw, dw, lane, s_ok, ea[j], eb[j]).m);
      }
    }
  }
  if (s_ok) a.blk[uint64_t(blockIdx.y) * a.n_src + (s - t.s_lo)] = n;
}

// a thread per source from the first one pass 1 counted
__global__ __launch_bounds__(256) void k_table_find_scan(FindArgs a) {
  const uint64_t i = uint64_t(a.bx0) * TT_WORDS * 64 + blockIdx.x * uint64_t(blockDim.x) + threadIdx.x;
  if (i >= a.n_src) return;
  unsigned long long run = 0;
  for (uint32_t by = 0; by < a.NB; by++) {
    unsigned long long* c = a.blk + uint64_t(by) * a.n_src + i;
    const unsigned long long n = *c;
    *c = run;
    run += n;
  }
  a.t.cnt[i] = run;
}

// Pass 2: a wave per (source word of the page, destination block).  Per destination word the lane's words of
// every slot go to a lane-private column of the buffer (LDS, or global scratch for many slots); the lane then
// walks its set destination bits in ascending order and under each the slots, which is the (d, k) order of its
// records.
template <bool CMP>
__global__ __launch_bounds__(64) void k_table_find_emit(FindArgs a) {
  extern __shared__ uint64_t find_lds[];
  const TileArgs& t = a.t;
  const uint32_t lane = threadIdx.x;
  // word x of slot kk: buf[(kk * 4 + x) * 64]
  uint64_t* buf = (a.scratch ? a.scratch + uint64_t(blockIdx.x) * t.nk * 256 : find_lds) + lane;
  const uint32_t sw_lo = a.s_from / 64;
  const uint64_t items = uint64_t((a.s_next + 63) / 64 - sw_lo) * a.NB;
  for (uint64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const uint32_t sw = sw_lo + uint32_t(item / a.NB), by = uint32_t(item % a.NB);
    const uint32_t s = sw * 64 + lane;
    const bool s_ok = s >= a.s_from && s < a.s_next;
    // the lane's records of this block: [off, end) of the page
    unsigned long long off = 0, end = 0;
    if (s_ok) {
      const uint64_t i = s - t.s_lo;
      const unsigned long long before = a.blk[uint64_t(by) * a.n_src + i];
      off = a.offs[s - a.s_from] + before;
      end = off + (by + 1 < a.NB ? a.blk[uint64_t(by + 1) * a.n_src + i] : t.cnt[i]) - before;
    }
    if (__ballot(off != end) == 0) continue;
    const uint32_t dw_end = min((by + 1) * TT_WORDS, t.W);
    for (uint32_t dw = by * TT_WORDS; dw < dw_end; dw++) {
      uint64_t u = 0;
      for (uint32_t kk = 0; kk < t.nk; kk++) {
        const uint64_t eg_at = (uint64_t(s - t.s_lo) * t.K + t.k_lo + kk) * t.W + dw;
        const FindWords f = find_words<CMP, true>(a, kk, sw, dw, lane, s_ok, s_ok ? t.a.eg[eg_at] : 0ull,
                                                  CMP && s_ok ? t.b.eg[eg_at] : 0ull);
        uint64_t* o = buf + uint64_t(kk) * 256;
        o[0] = f.m, o[64] = f.i, o[128] = f.e, o[192] = f.o;
        u |= f.m;
      }
      while (u) {
        const uint32_t b = uint32_t(__builtin_ctzll(u)), d = dw * 64 + b;
        u &= u - 1;
        for (uint32_t kk = 0; kk < t.nk; kk++) {
          const uint64_t* o = buf + uint64_t(kk) * 256;
          if (!((o[0] >> b) & 1)) continue;
          // the codes of cyc_table_cells (dev_query.hpp)
          const uint32_t k = t.k_lo + kk;
          const uint8_t sa = t.a.status[uint64_t(d) * t.K + k];
          const bool ai = (o[64] >> b) & 1, ae = (o[128] >> b) & 1;
          uint32_t ci, ce = CYC_CONN_UNKNOWN, co = 0;
          if (sa == CYC_JOB_VALID) {
            ci = ai ? CYC_CONN_ALLOWED : CYC_CONN_BLOCKED;
            ce = ae ? CYC_CONN_ALLOWED : CYC_CONN_BLOCKED;
          } else {
            ci = sa == CYC_JOB_BAD_PORT_PROTOCOL ? CYC_CONN_INVALID_PORT_PROTOCOL : CYC_CONN_INVALID_NAMED_PORT;
          }
          const uint32_t cc = sa == CYC_JOB_VALID ? (ai && ae ? CYC_CONN_ALLOWED : CYC_CONN_BLOCKED) : ci;
          if (CMP) {
            const uint8_t sb = t.b.status[uint64_t(d) * t.K + k];
            co = sb == CYC_JOB_VALID                ? ((o[192] >> b) & 1 ? CYC_CONN_ALLOWED : CYC_CONN_BLOCKED)
                 : sb == CYC_JOB_BAD_PORT_PROTOCOL ? CYC_CONN_INVALID_PORT_PROTOCOL
                 : sb == CYC_JOB_BAD_NAMED_PORT    ? CYC_CONN_INVALID_NAMED_PORT
                                                   : CYC_CONN_NO_JOB;
          }
          // (a record past the source's share would mean the planes changed between the passes)
          if (off < end) a.out[off] = make_uint4(s, d, k, ci | ce << 8 | cc << 16 | co << 24);
          off++;
        }
      }
    }
  }
}

}  // namespace cyc
