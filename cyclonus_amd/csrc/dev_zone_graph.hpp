// dev_zone_graph.hpp — the zone graph of a table (cyc_table_zone_graph): the condensation of the FROM closure reduced to
// its Hasse diagram.  The reference has no such summary.  Input: the closure plane C of dev_closure.hpp and rep[Z], the
// smallest pod of every zone in ascending order (the host numbers the zones from k_closure_zones' representatives).
//
//   k_zone_compress  C -> the zone reach plane R [Z][zpitch] (zpitch = Wz rounded up to 16 words, Wz = ceil(Z / 64)): a
//                    wave per (zone row a, zone word wz), lane i tests bit rep[64 wz + i] of row rep[a] (false at or
//                    beyond Z), the word is the wave's ballot.  The padding words come out zero the same way.
//   k_zone_cover     cover[a] = S[a] & ~(OR over c in S[a] of S[c]) with S = R without its diagonal: zone b stays in row a
//                    iff a reaches b and no third zone lies between them.  A block owns ZC_ROWS rows and ZC_CHUNK column
//                    words and walks every pivot word kb of R inside the one launch (R is constant: no pivot word
//                    depends on another, unlike the closure).  Per kb it stages the 64 pivot rows' chunk in the LDS, each
//                    pivot row's own bit cleared; a wave keeps the accumulators of its ZC_WAVE_ROWS rows in registers
//                    (a lane holds two neighbouring words: 16 bytes of a staged row), takes the rows' mask words
//                    R[a][kb] with one load (lane j = row j of the wave), clears bit a and walks each wave-uniform mask
//                    with ctz as k_closure_update does.  A pivot word in which no row of the block has a bit is not
//                    staged.  At the end S & ~acc is stored once.
//   k_zone_counts    the set bits of every cover row, a wave per row
//   k_zone_edges     a wave per row writes its edges (a, b) at the row's offset (the host's exclusive scan of the
//                    counts) in ascending b: 64 words a step, a wave prefix sum of their popcounts
//   k_zone_copy      R without its padding: [Z][zpitch] -> [Z][Wz]
// Every (row, word) and every edge has one writer, nothing is read that the same launch writes, no atomics: the same
// bits from run to run.
#pragma once

namespace cyc {

constexpr uint32_t ZC_CHUNK = 128;    // column words of a cover block: 64 x 128 words = 64 KiB of LDS, two blocks a CU
constexpr uint32_t ZC_THREADS = 512;  // 8 waves
constexpr uint32_t ZC_WAVE_ROWS = 16; // rows of a wave: 16 x 2 words of accumulators = 64 VGPRs
constexpr uint32_t ZC_ROWS = ZC_THREADS / 64 * ZC_WAVE_ROWS;  // rows of a cover block (128)

struct ZoneGraphArgs {
  uint32_t Z, Wz, zpitch;    // R, cover: [Z][zpitch], 16-byte aligned, zpitch a multiple of 16
  uint32_t pitch;            // of the closure plane
  const uint64_t* c;         // the FROM closure [P][pitch]
  const uint32_t* rep;       // [Z] ascending
  uint64_t* r;               // the zone reach plane
  uint64_t* cover;
  unsigned long long* cnt;   // [Z]: k_zone_counts' counts; k_zone_edges' offsets
  unsigned long long total;  // k_zone_edges: the number of edges
  int2* edges;               // [total]: (a, b)
};

__global__ __launch_bounds__(256) void k_zone_compress(ZoneGraphArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t n = uint64_t(a.Z) * a.zpitch, step = gridDim.x * uint64_t(blockDim.x / 64);
  for (uint64_t id = blockIdx.x * uint64_t(blockDim.x / 64) + (threadIdx.x >> 6); id < n; id += step) {  // (wave-uniform)
    const uint32_t row = uint32_t(id / a.zpitch), wz = uint32_t(id % a.zpitch), z = wz * 64 + lane;
    bool on = false;
    if (z < a.Z) {
      const uint32_t q = a.rep[z];
#ifndef CYC_DEFECT_ZONE_COMPRESS_WORD
      on = a.c[uint64_t(a.rep[row]) * a.pitch + q / 64] >> (q % 64) & 1;
#else  // (a planted defect of the tests: the bit is taken from word 0)
      on = a.c[uint64_t(a.rep[row]) * a.pitch] >> (q % 64) & 1;
#endif
    }
    const uint64_t word = __ballot(on);
    if (lane == 0) a.r[uint64_t(row) * a.zpitch + wz] = word;
  }
}

__global__ __launch_bounds__(ZC_THREADS) void k_zone_cover(ZoneGraphArgs a) {
  __shared__ ulonglong2 pan[64 * ZC_CHUNK / 2];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t c0 = blockIdx.x * ZC_CHUNK, cn = min(ZC_CHUNK, a.zpitch - c0);  // (zpitch is even: cn too)
  const uint32_t r0 = blockIdx.y * ZC_ROWS + wave * ZC_WAVE_ROWS;                // the wave's first row
  const uint32_t w = lane * 2;
  const bool in_row = w < cn;
  const uint32_t my_row = r0 + lane;  // lanes below ZC_WAVE_ROWS fetch the mask words of the wave's rows
  const bool mask_lane = lane < ZC_WAVE_ROWS && my_row < a.Z;
  ulonglong2 acc[ZC_WAVE_ROWS];
#pragma unroll
  for (uint32_t j = 0; j < ZC_WAVE_ROWS; j++) acc[j] = ulonglong2{0, 0};
#ifndef CYC_DEFECT_ZONE_LAST_WORD
  const uint32_t kb_end = a.Wz;
#else  // (a planted defect of the tests: the last pivot word is left out)
  const uint32_t kb_end = a.Wz - 1;
#endif
  for (uint32_t kb = 0; kb < kb_end; kb++) {
    uint64_t mv = mask_lane ? a.r[uint64_t(my_row) * a.zpitch + kb] : 0ull;
#ifndef CYC_DEFECT_ZONE_MASK_SELF  // (a planted defect of the tests: the mask keeps the row's own bit)
    if (my_row / 64 == kb) mv &= ~(uint64_t(1) << (my_row % 64));
#endif
    // (the barrier also ends the last step's reads of the LDS)
    if (!__syncthreads_or(mv != 0)) continue;
    // the block's chunk of the 64 pivot rows, 16 bytes a thread; a pivot at or beyond Z and the words at or beyond cn
    // are staged as zero
    for (uint32_t i = tid; i < 64 * (ZC_CHUNK / 2); i += ZC_THREADS) {
      const uint32_t k = i / (ZC_CHUNK / 2), x = i % (ZC_CHUNK / 2) * 2, piv = kb * 64 + k;
      ulonglong2 v{0, 0};
      if (x < cn && piv < a.Z) {
        v = *reinterpret_cast<const ulonglong2*>(a.r + uint64_t(piv) * a.zpitch + c0 + x);
#ifndef CYC_DEFECT_ZONE_PIVOT_SELF  // (a planted defect of the tests: the staged pivot row keeps its own bit)
        if (c0 + x == kb) v.x &= ~(uint64_t(1) << k);
        if (c0 + x + 1 == kb) v.y &= ~(uint64_t(1) << k);
#endif
      }
      pan[i] = v;
    }
    __syncthreads();
#pragma unroll
    for (uint32_t j = 0; j < ZC_WAVE_ROWS; j++) {
      uint64_t m = lane_word(mv, j);  // (wave-uniform)
      while (m) {
        const ulonglong2 v = pan[uint32_t(__builtin_ctzll(m)) * (ZC_CHUNK / 2) + lane];
        acc[j].x |= v.x, acc[j].y |= v.y;
        m &= m - 1;
      }
    }
  }
  if (!in_row) return;
#pragma unroll
  for (uint32_t j = 0; j < ZC_WAVE_ROWS; j++) {
    const uint32_t row = r0 + j;
    if (row >= a.Z) break;
    ulonglong2 s = *reinterpret_cast<const ulonglong2*>(a.r + uint64_t(row) * a.zpitch + c0 + w);
    if (c0 + w == row / 64) s.x &= ~(uint64_t(1) << (row % 64));
    if (c0 + w + 1 == row / 64) s.y &= ~(uint64_t(1) << (row % 64));
    s.x &= ~acc[j].x, s.y &= ~acc[j].y;
    *reinterpret_cast<ulonglong2*>(a.cover + uint64_t(row) * a.zpitch + c0 + w) = s;
  }
}

__global__ __launch_bounds__(256) void k_zone_counts(ZoneGraphArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t row = blockIdx.x * uint64_t(blockDim.x / 64) + (threadIdx.x >> 6);
  if (row >= a.Z) return;
  uint32_t n = 0;
  for (uint32_t w = lane; w < a.Wz; w += 64) n += __popcll(a.cover[row * a.zpitch + w]);
#pragma unroll
  for (int m = 32; m; m >>= 1) n += __shfl_xor(n, m, 64);
  if (lane == 0) a.cnt[row] = n;
}

__global__ __launch_bounds__(256) void k_zone_edges(ZoneGraphArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t row = blockIdx.x * uint64_t(blockDim.x / 64) + (threadIdx.x >> 6);
  if (row >= a.Z) return;
#ifndef CYC_DEFECT_ZONE_OFFSET
  unsigned long long at = a.cnt[row];
#else  // (a planted defect of the tests: the inclusive scan, which is the next row's offset; the last row writes nothing)
  if (row + 1 >= a.Z) return;
  unsigned long long at = a.cnt[row + 1];
#endif
  for (uint32_t w0 = 0; w0 < a.Wz; w0 += 64) {
    uint64_t x = w0 + lane < a.Wz ? a.cover[row * a.zpitch + w0 + lane] : 0ull;
    const uint32_t n = __popcll(x);
    uint32_t before = n;  // the inclusive prefix sum over the lanes, then without the lane's own
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t v = __shfl_up(before, d, 64);
      if (lane >= uint32_t(d)) before += v;
    }
    const uint32_t all = __shfl(before, 63, 64);
    unsigned long long o = at + (before - n);
    for (; x; x &= x - 1, o++)
      if (o < a.total) a.edges[o] = int2{int(row), int((w0 + lane) * 64 + uint32_t(__builtin_ctzll(x)))};  // (never beyond the list)
    at += all;
  }
}

// R without its padding: [Z][zpitch] -> [Z][Wz] (8-byte aligned), a word a thread at a time.
__global__ __launch_bounds__(256) void k_zone_copy(ZoneGraphArgs a, uint64_t* out) {
  const uint64_t n = uint64_t(a.Z) * a.Wz, step = gridDim.x * uint64_t(blockDim.x);
  for (uint64_t i = blockIdx.x * uint64_t(blockDim.x) + threadIdx.x; i < n; i += step) out[i] = a.r[i / a.Wz * a.zpitch + i % a.Wz];
}

}  // namespace cyc
