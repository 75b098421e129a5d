// Exact k-nearest neighbours in a low-dimensional space (spv_knn; spVIPES.latent_neighbors of the user API): for every query row the
// k candidates with the smallest (squared Euclidean distance, candidate index), nothing of size queries x candidates ever stored.
//
// How the work is laid out on the chip
//   * The scan -- one query per lane, the grid (query tiles) x (chunks), the chunk passing through LDS a tile at a time, the chains in
//     flight per lane -- is pair_scan of spv_pair_scan.h, which states the layout.  The chunks are chosen so that a few workgroups per
//     CU exist when the query tiles alone do not fill the chip (knn_splits).
//   * A pair (d, j) is ONE 64-bit key, the bits of d above j: d is never negative and never NaN where a key is made, so unsigned order
//     of the keys is the order (d, j).  Per candidate the lane pays DP subtracts, DP fmas and the compare against the key of its
//     current worst entry, kept in registers.
//   * Only a hit touches the lane's entries, which live in LDS as [slot][lane] keys (k rounded up to a multiple of 8, x 128 x 8 bytes: 16 / 32 / 64 KiB at
//     k = 16 / 32 / 64, next to the 4 / 8 / 16 KiB tile).  During the scan they are an UNSORTED set: a hit overwrites the worst entry and the
//     new worst is found by one pass of independent 8-byte reads, eight in flight at a time (knn_keep).  Keeping the set sorted instead costs a chain of
//     dependent LDS round trips per hit, k / 2 of them on average, and with about k ln(n / k) hits per query -- most candidates hit in
//     SOME lane of a wave -- that chain was the whole cost at k = 50.  The set is sorted once, at the end.
//   * n_split > 1: every (query tile, chunk) writes its sorted keys into the workspace and knn_merge_kernel, one lane per query
//     again, merges the chunks' lists in the same order.  n_split == 1 writes the result directly: one launch.
// The result is a function of the pairs' distances and indices alone: a distance is one fixed fp32 chain per pair (knn_step), the
// order (d, j) is total, so neither the tiling nor the chunking nor the other queries of a call can change a bit of it.
//
// The part between the two KNN-CORE marks is plain C++ apart from __host__ __device__ and the two rounding intrinsics:
// tools/knn_host_check.py compiles exactly that text for the CPU.
#pragma once
#include "spv_common.h"
#include <cmath>

namespace spv {

// ---- KNN-CORE-BEGIN ----
constexpr int KNN_TQ = 128;        // queries per workgroup (one per lane)
constexpr int KNN_TC = 64;         // candidates per LDS tile (a multiple of KNN_CAND)
constexpr int KNN_CAND = 4;        // candidates in flight per lane (2 at DP = 64: see pair_scan)
constexpr int KNN_DMAX = 64;       // SPV_KNN_DMAX
constexpr int KNN_KMAX = 64;       // SPV_KNN_KMAX
constexpr int KNN_SPLIT_MAX = 64;  // SPV_KNN_SPLIT_MAX
constexpr int KNN_TARGET_WG = 1024;   // workgroups the chunks aim at: 4 per CU
constexpr int KNN_MIN_TILES = 4;      // a chunk is not worth fewer LDS tiles of candidates

typedef unsigned long long knn_key_t;
constexpr knn_key_t KNN_EMPTY = 0x7F800000FFFFFFFFull;   // (+inf, -1): an empty slot, after every key that can be made

// one term of the distance: u = q - c (one rounding), acc = fma(u, u, acc) (one rounding)
__host__ __device__ __forceinline__ float knn_step(float acc, float q, float c) {
  const float u = __fsub_rn(q, c);
  return __fmaf_rn(u, u, acc);
}

// the whole chain for one pair, t ascending from acc = +0
__host__ __device__ __forceinline__ float knn_d2(const float* q, const float* c, int D) {
  float acc = 0.f;
  for (int t = 0; t < D; ++t) acc = knn_step(acc, q[t], c[t]);
  return acc;
}

// (d, j) as one word, for +0 <= d < +inf (the chain never yields -0) and j >= 0: key order is the order (d, j)
__host__ __device__ __forceinline__ knn_key_t knn_key(float d, int j) {
  return ((knn_key_t)__builtin_bit_cast(unsigned, d) << 32) | (knn_key_t)(unsigned)j;
}
__host__ __device__ __forceinline__ float knn_key_d(knn_key_t key) { return __builtin_bit_cast(float, (unsigned)(key >> 32)); }
__host__ __device__ __forceinline__ int knn_key_j(knn_key_t key) { return (int)(unsigned)key; }

// (d, j) goes ahead of the entry `worst`: a distance that is not < +inf (overflow, NaN) never does
__host__ __device__ __forceinline__ bool knn_better(float d, int j, knn_key_t worst) { return d < INFINITY && knn_key(d, j) < worst; }

// ---- paging (spv_knn_paged): page p of a query's list is its columns [64 p, 64 p + 64), the best KNN_KMAX keys AFTER the last key of
// page p - 1.  The whole key is compared, not d alone: a group of equal distances that straddles a page boundary splits by index.
// A page that ended in an empty slot has `after` = KNN_EMPTY, which no key that can be made exceeds: such a query gets nothing more.
constexpr int KNN_PAGED_KMAX = 256;   // SPV_KNN_PAGED_KMAX
__host__ __device__ __forceinline__ bool knn_after(float d, int j, knn_key_t after) { return knn_key(d, j) > after; }
// the key a page's last column holds, from the row of idx / dist as it was written (-1 / +inf gives KNN_EMPTY)
__host__ __device__ __forceinline__ knn_key_t knn_after_key(float d, int j) { return knn_key(d, j); }
// columns of page p for k columns in all
__host__ __device__ __forceinline__ int knn_page_cols(int k, int p) { return k - p * KNN_KMAX < KNN_KMAX ? k - p * KNN_KMAX : KNN_KMAX; }

// k empty slots at stride `st`
__host__ __device__ __forceinline__ void knn_clear(knn_key_t* list, int st, int k) {
  for (int s = 0; s < k; ++s) list[s * st] = KNN_EMPTY;
}

// ---- during the scan: an unsorted set of the best `fill` <= k keys seen, its worst one known once it is full
struct KnnTop { knn_key_t worst; int wpos, fill; };
__host__ __device__ __forceinline__ void knn_top_init(KnnTop& t) { t.worst = KNN_EMPTY; t.wpos = 0; t.fill = 0; }

// the set's slots: k rounded up to a multiple of KNN_SCAN; the slots from k on hold key 0, which is never the worst of a full set
constexpr int KNN_SCAN = 8;   // keys read per round of the worst-entry pass: independent reads, in flight together
__host__ __device__ __forceinline__ int knn_slots(int k) { return (k + KNN_SCAN - 1) / KNN_SCAN * KNN_SCAN; }
__host__ __device__ __forceinline__ void knn_pad(knn_key_t* list, int st, int k) {
  for (int s = k; s < knn_slots(k); ++s) list[s * st] = 0;
}

// `key`, known to go ahead of t.worst, joins the set: into the next free slot, or over the worst entry; a full set then finds its new
// worst entry (keys are distinct, one per candidate, so only a set of one can have the key 0 as its worst: slot 0 then, as found)
__host__ __device__ __forceinline__ void knn_keep(KnnTop& t, knn_key_t* list, int st, int k, knn_key_t key) {
  const int s = t.fill < k ? t.fill++ : t.wpos;
  list[s * st] = key;
  if (t.fill < k) return;
  knn_key_t w = list[0];
  int p = 0;
  for (int e0 = 0; e0 < k; e0 += KNN_SCAN) {
    knn_key_t v[KNN_SCAN];
#pragma unroll
    for (int u = 0; u < KNN_SCAN; ++u) v[u] = list[(e0 + u) * st];
#pragma unroll
    for (int u = 0; u < KNN_SCAN; ++u)
      if (v[u] > w) { w = v[u]; p = e0 + u; }
  }
  t.worst = w;
  t.wpos = p;
}

// ---- sorted lists
// `key`, which goes ahead of the ascending list's last entry or IS that entry, takes its place; the last entry drops out
__host__ __device__ __forceinline__ void knn_insert(knn_key_t* list, int st, int k, knn_key_t key) {
  int s = k - 1;
  while (s > 0 && key < list[(s - 1) * st]) {
    list[s * st] = list[(s - 1) * st];
    --s;
  }
  list[s * st] = key;
}

// the first n entries into ascending order (insertion sort: once per lane and chunk)
__host__ __device__ __forceinline__ void knn_sort(knn_key_t* list, int st, int n) {
  for (int e = 1; e < n; ++e) knn_insert(list, st, e + 1, list[e * st]);
}

// an ascending list of k keys (contiguous) merged into the ascending list: once one of its entries fails, the rest do
__host__ __device__ __forceinline__ void knn_merge(knn_key_t* list, int st, int k, const knn_key_t* part) {
  for (int e = 0; e < k; ++e) {
    if (!(part[e] < list[(k - 1) * st])) break;
    knn_insert(list, st, k, part[e]);
  }
}

// chunks of the candidates = workgroups per query tile; a pure function of the shapes
inline int knn_splits(int n_q, int n_c) {
  if (n_q < 1 || n_c < 1) return 1;
  const int tiles = (n_q + KNN_TQ - 1) / KNN_TQ;
  if (2 * tiles >= KNN_TARGET_WG) return 1;   // two query tiles per CU: the queries alone fill the chip
  int s = (KNN_TARGET_WG + tiles - 1) / tiles;
  const int most = n_c / (KNN_MIN_TILES * KNN_TC);
  if (s > most) s = most;
  if (s > KNN_SPLIT_MAX) s = KNN_SPLIT_MAX;
  return s < 1 ? 1 : s;
}

// candidates per chunk: chunk c owns [c * per, min((c + 1) * per, n_c)), possibly nothing
inline int knn_chunk(int n_c, int n_split) { return (int)(((long long)n_c + n_split - 1) / n_split); }
// ---- KNN-CORE-END ----

}  // namespace spv
#include "spv_pair_scan.h"   // the scan, on the constants and knn_step above
namespace spv {

struct KnnArgs {
  const float* Q; long ld_q; int n_q;
  const float* C; long ld_c; int n_c;
  int D, k;
  const int* exclude;
  int n_split, per;          // chunks, candidates per chunk
  int* idx; float* dist; int ld_out;
  knn_key_t* ws;             // [n_split][n_q][k] keys (n_split > 1)
};

constexpr int knn_lds_bytes(int DP, int k) { return KNN_TC * DP * 4 + (k + KNN_SCAN - 1) / KNN_SCAN * KNN_SCAN * KNN_TQ * 8; }

// query i's sorted keys as its row of idx / dist
__device__ __forceinline__ void knn_write_row(const KnnArgs& a, int i, const knn_key_t* list) {
  const int o = i * a.ld_out;
  for (int s = 0; s < a.k; ++s) { const knn_key_t key = list[s * KNN_TQ]; a.dist[o + s] = knn_key_d(key); a.idx[o + s] = knn_key_j(key); }
}

// grid (query tiles, n_split), KNN_TQ threads, knn_lds_bytes(DP, k) of dynamic LDS.  The compiler issues a round's CAND x DP tile
// reads ahead of its arithmetic and keeps the eight keys of a worst-entry round next to them: 96 registers at DP = 16, 176 at DP = 32
// and, with two candidates in flight, 208 at DP = 64, no scratch -- 2 waves per SIMD for the two larger forms, i.e. 4 workgroups per
// CU (the LDS allows that up to k = 32 at DP = 32).  The bound keeps any later form from going past 256.
// PAGED (spv_knn_paged, pages >= 1): a.idx / a.dist point at the page's first column and a.k is the page's width; the query's `after`
// key is read from the column just before it, which the previous page wrote (this launch writes only columns >= 0 of the page, or the
// workspace: no overlap), and a candidate is offered only if knn_after.  The flag is a compile-time one: the forms without it are the
// code they were.  The paged forms carry the 64-bit key: 105 / 178 / 210 registers, no scratch
// (4 / 2 / 2 waves per SIMD).
template <int DP, bool PAGED = false>
__global__ __launch_bounds__(KNN_TQ) __attribute__((amdgpu_waves_per_eu(2))) void knn_partial_kernel(const KnnArgs a) {
  extern __shared__ __align__(16) float knn_lds[];
  float* const tile = knn_lds;                                                             // [KNN_TC][DP]
  knn_key_t* const list = reinterpret_cast<knn_key_t*>(knn_lds + KNN_TC * DP) + threadIdx.x;   // [k][KNN_TQ], this lane's column
  const int lane = threadIdx.x, i = blockIdx.x * KNN_TQ + lane, k = a.k;
  const bool live = i < a.n_q;

  float q[DP];
  scan_load_query<DP>(a, i, live, q);
  const int ex = (live && a.exclude) ? a.exclude[i] : -1;
  knn_key_t after = KNN_EMPTY;   // a lane without a query is offered nothing
  if (PAGED && live) after = knn_after_key(a.dist[i * a.ld_out - 1], a.idx[i * a.ld_out - 1]);
  knn_clear(list, KNN_TQ, k);
  knn_pad(list, KNN_TQ, k);
  KnnTop top;
  knn_top_init(top);

  pair_scan<DP>(a, q, tile, [&](int j, int, bool in, float d2) {   // rows past the chunk's end: computed, never offered
    if (PAGED) {
      if (in && j != ex && knn_better(d2, j, top.worst) && knn_after(d2, j, after)) knn_keep(top, list, KNN_TQ, k, knn_key(d2, j));
    } else {
      if (in && j != ex && knn_better(d2, j, top.worst)) knn_keep(top, list, KNN_TQ, k, knn_key(d2, j));
    }
  });
  if (!live) return;
  knn_sort(list, KNN_TQ, top.fill);
  if (a.n_split == 1) knn_write_row(a, i, list);
  else {
    const int o = ((int)blockIdx.y * a.n_q + i) * k;
    for (int s = 0; s < k; ++s) a.ws[o + s] = list[s * KNN_TQ];
  }
}

// grid (query tiles), KNN_TQ threads, k * KNN_TQ * 8 bytes of dynamic LDS: the chunks' lists in chunk order into one list
__global__ __launch_bounds__(KNN_TQ) void knn_merge_kernel(const KnnArgs a) {
  extern __shared__ __align__(16) float knn_lds[];
  const int i = blockIdx.x * KNN_TQ + threadIdx.x, k = a.k;
  if (i >= a.n_q) return;
  knn_key_t* const list = reinterpret_cast<knn_key_t*>(knn_lds) + threadIdx.x;
  knn_clear(list, KNN_TQ, k);
  for (int c = 0; c < a.n_split; ++c) knn_merge(list, KNN_TQ, k, a.ws + (c * a.n_q + i) * k);
  knn_write_row(a, i, list);
}

}  // namespace spv
