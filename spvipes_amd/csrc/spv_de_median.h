// Differential expression, the exact per-gene median of lfc_m = de_lfc(x1, x2, eps) over the pairs (spv_de_median): the two middle
// order statistics, ranks (n_pairs - 1) / 2 and n_pairs / 2, of the very fp32 numbers de_pairs_kernel (spv_de.h) reduces.
//
// A median is a selection, not a streaming reduction, and n_pairs x n_genes values are never stored (670 GB at the limits).  The
// kernel is a radix select over the order-preserving uint32 image of the lfc (dm_key), 8 bits per pass, most significant first:
// FOUR gather passes, each re-gathering the bank rows and recomputing the lfc exactly as de_pairs_kernel does, and a small
// per-gene "pick" kernel after each.
//   * de_median_pass_kernel<PASS>: lanes run along genes, a pair's two row numbers are wave-uniform, DE_UNROLL pairs are in flight
//     per wave, workgroups of one gene tile land on one XCD -- all as in de_pairs_kernel.  A workgroup is DM_WAVES = 16 waves on one
//     gene tile and one split of the pairs; its waves share ONE LDS histogram [256 bins][64 lanes] of uint32 (64 KiB, two
//     workgroups = 32 waves per CU).  A lane counts only its own gene's keys whose leading 8 * PASS bits equal the prefix found so
//     far, into the column of the histogram that only lanes of its gene touch: bank = lane mod 32, so a wave's update is conflict
//     free, and the waves' updates to one counter are LDS integer atomics.  The non-zero counters are then added to the global
//     histogram [256][n_genes] with integer atomics (in the later passes almost every counter is zero).  Every counter is uint32:
//     2^24 + 1 and more fits whatever the split.
//   * de_median_pick_kernel: per gene, the bin that holds the wanted rank; the rank is rebased into the bin, the prefix grows by 8
//     bits and the global histogram is zeroed again.
//   * The second middle value costs no pass of its own.  While both ranks fall into the same bin nothing is to be done.  Where they
//     part -- rank r is the last of its bin -- the upper one is the SMALLEST key of the next non-empty bin: that bin's prefix is
//     handed to the next pass, whose lanes take min(key) over the keys that carry it (a register, merged by an integer atomic min),
//     and the value is final.  Parting in the last pass needs nothing: the bin is the key.
// Integer atomics only: the result does not depend on the order of arrival, two calls agree bit for bit.  -0.0 is counted as +0.0.
#pragma once
#include "spv_de.h"

namespace spv {

constexpr int DM_WAVES = 16;          // waves per workgroup of de_median_pass_kernel
constexpr int DM_BINS = 256;          // 8 bits per pass
constexpr int DM_PASSES = 4;
constexpr int DM_TARGET_WGS = 512;    // two 64 KiB workgroups per CU
constexpr int DM_STATE = 5;           // uint32 words per gene beside the histogram: prefix, rank, upper mode, upper key, running min
constexpr unsigned DM_NONE = 0xffffffffu;

struct DmArgs {
  const float *bank1, *bank2; long ld1, ld2;
  const int *rows1, *rows2; int n_rows1, n_rows2;
  int n_genes, n_pairs; float eps;
  float* mid; long ld_mid;
  unsigned* ws; int splits;
};

// workspace words: hist[256][n_genes], then prefix, rank, mode, upper key, running min: [n_genes] each
inline long dm_ws_words(int n_genes) { return (long)(DM_BINS + DM_STATE) * n_genes; }

// splits of the pairs = workgroups per gene tile: one round of workgroups on the chip, never fewer than DE_MIN_PAIRS pairs per wave
inline int dm_splits(int n_genes, int n_pairs) {
  const int tiles = (n_genes + 63) / 64;
  int s = DM_TARGET_WGS / tiles > 1 ? DM_TARGET_WGS / tiles : 1;
  const int most = n_pairs / (DM_WAVES * DE_MIN_PAIRS) > 1 ? n_pairs / (DM_WAVES * DE_MIN_PAIRS) : 1;
  return s < most ? s : most;   // (>= 1, and <= n_pairs)
}

// fp32 -> uint32, order preserving: negatives have all bits flipped, the others get the sign bit; -0.0 is taken as +0.0
__device__ __forceinline__ unsigned dm_key(float f) {
  const unsigned u = __float_as_uint(f);
  if (u == 0x80000000u) return 0x80000000u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float dm_value(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

template <int PASS>
__device__ __forceinline__ void dm_count(unsigned* col, unsigned& mn, float x1, float x2, float eps, unsigned pre, unsigned hip) {
  const unsigned key = dm_key(de_lfc(x1, x2, eps));
  if (PASS == 0) {
    atomicAdd(col + (key >> 24) * 64, 1u);
  } else {
    const unsigned top = key >> (32 - 8 * PASS);
    if (top == pre) atomicAdd(col + ((key >> (24 - 8 * PASS)) & 255u) * 64, 1u);
    if (top == hip) mn = min(mn, key);
  }
}

__global__ __launch_bounds__(256) void de_median_zero_kernel(unsigned* p, long n) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) p[i] = 0u;
}

template <int PASS>
__global__ __launch_bounds__(64 * DM_WAVES) void de_median_pass_kernel(DmArgs a) {
  __shared__ unsigned hist[DM_BINS * 64];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int tiles = (a.n_genes + 63) >> 6, nwg = tiles * a.splits;
  // workgroup ids id, id + 8, id + 16, ... share an XCD: give them consecutive work items (the grid is a multiple of 8)
  const int per = gridDim.x >> 3, w = (blockIdx.x & 7) * per + (blockIdx.x >> 3);
  if (w >= nwg) return;   // (the whole workgroup: no barrier is skipped by a part of it)
  const int tile = w / a.splits, split = w - tile * a.splits;
  const int col = tile * 64 + lane, j = min(col, a.n_genes - 1);   // a lane beyond the last gene re-reads it and publishes nothing
  for (int i = threadIdx.x; i < DM_BINS * 64; i += 64 * DM_WAVES) hist[i] = 0u;
  const long g = a.n_genes;
  unsigned* const state = a.ws + DM_BINS * g;
  unsigned pre = 0u, hip = DM_NONE, mn = DM_NONE;
  if (PASS > 0) {
    pre = state[j] >> (32 - 8 * PASS);
    if (state[2 * g + j] == 1u) hip = state[3 * g + j] >> (32 - 8 * PASS);   // (a prefix of 8 * PASS <= 24 bits never equals DM_NONE)
  }
  __syncthreads();
  // this wave's pairs: the split's share [p0, p1) cut in DM_WAVES
  const int p0 = (int)((long)split * a.n_pairs / a.splits), p1 = (int)((long)(split + 1) * a.n_pairs / a.splits);
  const int m0 = p0 + (int)((long)wave * (p1 - p0) / DM_WAVES), m1 = p0 + (int)((long)(wave + 1) * (p1 - p0) / DM_WAVES);
  const float* const b1 = a.bank1 + j;
  const float* const b2 = a.bank2 + j;
  unsigned* const mine = hist + lane;
  int m = m0;
  for (; m + DE_UNROLL <= m1; m += DE_UNROLL) {
    float x1[DE_UNROLL], x2[DE_UNROLL];
#pragma unroll
    for (int u = 0; u < DE_UNROLL; ++u) {
      x1[u] = b1[de_row(a.rows1, m + u, a.n_rows1, a.ld1)];
      x2[u] = b2[de_row(a.rows2, m + u, a.n_rows2, a.ld2)];
    }
#pragma unroll
    for (int u = 0; u < DE_UNROLL; ++u) dm_count<PASS>(mine, mn, x1[u], x2[u], a.eps, pre, hip);
  }
  for (; m < m1; ++m)
    dm_count<PASS>(mine, mn, b1[de_row(a.rows1, m, a.n_rows1, a.ld1)], b2[de_row(a.rows2, m, a.n_rows2, a.ld2)], a.eps, pre, hip);
  if (PASS > 0 && mn != DM_NONE && col < a.n_genes) atomicMin(state + 4 * g + col, mn);
  __syncthreads();
  for (int i = threadIdx.x; i < DM_BINS * 64; i += 64 * DM_WAVES) {   // i = bin * 64 + lane: consecutive threads, consecutive genes
    const unsigned c = hist[i];
    const int cc = tile * 64 + (i & 63);
    if (c != 0u && cc < a.n_genes) atomicAdd(a.ws + (long)(i >> 6) * g + cc, c);
  }
}

// one workgroup of 4 waves per gene tile: all four stage the tile's 256 x 64 counters in LDS (and zero them in the workspace for
// the next pass), DM_PICK_LOADS independent loads at a time; wave 0 walks the bins without a branch, so that its LDS reads pipeline
constexpr int DM_PICK_LOADS = 16;
__global__ __launch_bounds__(256) void de_median_pick_kernel(DmArgs a, int pass) {
  __shared__ unsigned hist[DM_BINS * 64];
  const long g = a.n_genes;
  const int base = blockIdx.x * 64;
  const int cc = base + ((int)threadIdx.x & 63);   // (256 is a multiple of 64: a thread stays on one gene)
  const bool live = cc < a.n_genes;
  for (int i0 = threadIdx.x; i0 < DM_BINS * 64; i0 += 256 * DM_PICK_LOADS) {
    unsigned c[DM_PICK_LOADS];
#pragma unroll
    for (int u = 0; u < DM_PICK_LOADS; ++u) c[u] = live ? a.ws[(long)((i0 + 256 * u) >> 6) * g + cc] : 0u;
#pragma unroll
    for (int u = 0; u < DM_PICK_LOADS; ++u) {
      hist[i0 + 256 * u] = c[u];
      if (live && pass + 1 < DM_PASSES) a.ws[(long)((i0 + 256 * u) >> 6) * g + cc] = 0u;
    }
  }
  __syncthreads();
  const int col = base + (int)threadIdx.x;
  if (threadIdx.x >= 64 || col >= a.n_genes) return;
  unsigned* const state = a.ws + DM_BINS * g + col;
  // upper value: 0 = still in the lower one's bin, 1 = pending (hik is its prefix), 2 = settled (hik is its key), 3 = not wanted (odd n_pairs)
  unsigned pre = 0u, r = (unsigned)((a.n_pairs - 1) / 2), mode = (a.n_pairs & 1) ? 3u : 0u, hik = 0u;
  if (pass > 0) { pre = state[0]; r = state[g]; mode = state[2 * g]; hik = state[3 * g]; }
  if (mode == 1u) { hik = state[4 * g]; mode = 2u; }   // the smallest key under the pending prefix, found by the pass before
  const int shift = 24 - 8 * pass;
  const unsigned* const mine = hist + threadIdx.x;
  // b = the bin with before <= r < before + cb (the counts under the prefix sum to more than r; the last bin otherwise),
  // nxt = the next non-empty bin after it (the last bin if there is none)
  unsigned cum = 0u, before = 0u, cb = 0u;
  int b = -1, nxt = -1;
#pragma unroll 16
  for (int bin = 0; bin < DM_BINS; ++bin) {
    const unsigned c = mine[bin * 64];
    if (b >= 0 && nxt < 0 && c != 0u) nxt = bin;
    if (b < 0 && (r < cum + c || bin == DM_BINS - 1)) { b = bin; before = cum; cb = c; }
    cum += c;
  }
  if (nxt < 0) nxt = DM_BINS - 1;
  if (mode == 0u && r + 1u >= before + cb) {   // rank r is the last of its bin: the upper value is the smallest key of the next non-empty bin
    hik = pre | ((unsigned)nxt << shift);
    mode = pass + 1 < DM_PASSES ? 1u : 2u;
  }
  pre |= (unsigned)b << shift;
  r -= before;
  if (pass + 1 < DM_PASSES) {
    state[0] = pre; state[g] = r; state[2 * g] = mode; state[3 * g] = hik; state[4 * g] = DM_NONE;
  } else {
    a.mid[col] = dm_value(pre);
    a.mid[a.ld_mid + col] = dm_value(mode == 2u ? hik : pre);
  }
}

}  // namespace spv
