// Entropic optimal transport between two point clouds in a low-dimensional space, nothing of size queries x candidates ever stored
// (spv_ot_softmin / spv_ot_topk; spVIPES.compute_transport_plan of the user API).  Both kernels are spv_knn's scan (spv_knn.h) with
// another reduction: the cost c_ij is knn_d2's fixed fp32 chain, bit for bit the distance latent_neighbors reports, and because
// u and -u square alike c(x_i, y_j) and c(y_j, x_i) are the same bits -- the two directions of a Sinkhorn iteration see one cost.
//
//   t_ij = fmaf(-c_ij, s, h_j)          one rounding; s = 1 / epsilon, h_j = psi_j + log b_j from the caller
//
//   * ot_softmin_kernel: L_i = log sum_j exp(t_ij) as a running (m, sum) pair per lane, sum = sum_j exp(t_j - m), m the largest t so
//     far.  One exp per candidate: e = exp(-|t - m|), then sum = fma(sum, e, 1), m = t for t > m and sum += e otherwise (ot_update).
//     A t that is not finite (h_j = -inf: a candidate without mass; a cost that overflowed; NaN) contributes nothing; a query without a
//     contributing candidate, n_c = 0 included, gets -inf.
//   * ot_topk_kernel: the k candidates with the largest t_ij, equal t to the smaller j, a non-finite t never.  The selection is
//     knn_keep / knn_sort / knn_merge on a 64-bit key whose UNSIGNED order is (t descending, j ascending): the usual sign-flip map of
//     the float's bits, complemented, above j (ot_key).  val = exp(t + r_i) with r_i = phi_i + log a_i is the plan entry itself;
//     mass_i is the sum of the row's kept val in list order.
//   * Layout: pair_scan of spv_pair_scan.h, which states it (one query per lane, the grid (query tiles) x (chunks), the chunk through
//     LDS a tile at a time), with the tile's h staged behind the tile; the chunk count is knn_splits' pure function of the shapes.
//   * n_split > 1: every (query tile, chunk) writes its (m, sum) pairs / its sorted keys to the workspace and a merge kernel, one lane
//     per query again, folds them IN CHUNK ORDER.  No floating-point atomics anywhere.
// What is reproducible: for fixed (shapes, n_split) two calls agree bit for bit, for both kernels.  idx of ot_topk is a function of the
// t bits alone: neither the tiling nor the chunking nor the other queries of a call change it, and val / mass follow from idx.  L of
// ot_softmin under DIFFERENT n_split agrees only within its error bound (tests/test_gpu_ot.py derives it), not bit for bit: the
// grouping of a sum changes its rounding.
//
// The part between the two OT-CORE marks is plain C++ apart from __host__ __device__, the rounding intrinsic and ot_exp:
// tools/ot_host_check.py compiles exactly that text, after the KNN-CORE text it builds on, for the CPU.
#pragma once
#include "spv_knn.h"

namespace spv {

// exp of a non-positive argument for the running sums: v_exp_f32 of x * log2(e) on the device
__host__ __device__ __forceinline__ float ot_exp(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __expf(x);
#else
  return expf(x);
#endif
}

// ---- OT-CORE-BEGIN ----
// t of one pair: -c * s + h with one rounding
__host__ __device__ __forceinline__ float ot_t(float c, float s, float h) { return __fmaf_rn(-c, s, h); }
__host__ __device__ __forceinline__ bool ot_finite(float t) { return fabsf(t) < INFINITY; }   // false for NaN

// ---- log-sum-exp: sum = sum_j exp(t_j - m) over the finite t seen, m their maximum; (-inf, 0) before the first one
struct OtLse { float m, sum; };
__host__ __device__ __forceinline__ void ot_lse_init(OtLse& a) { a.m = -INFINITY; a.sum = 0.f; }

// one more term.  The first finite t meets m = -inf: d = +inf, e = exp(-inf) = 0, sum = fma(0, 0, 1) = 1, m = t.
__host__ __device__ __forceinline__ void ot_update(OtLse& a, float t) {
  if (!ot_finite(t)) return;
  const float d = t - a.m;
  const float e = ot_exp(-fabsf(d));
  if (d > 0.f) { a.sum = __fmaf_rn(a.sum, e, 1.f); a.m = t; }
  else a.sum += e;
}

// the state of a later chunk joins: the larger m stays, the other sum is scaled to it.  An empty state (-inf, 0) changes nothing, and
// joining a state to an empty one copies it (exp(-inf) = 0, fma(0, 0, sum) = sum).
__host__ __device__ __forceinline__ void ot_merge(OtLse& a, OtLse p) {
  if (p.m > a.m) { a.sum = __fmaf_rn(a.sum, ot_exp(a.m - p.m), p.sum); a.m = p.m; }
  else if (p.sum > 0.f) a.sum = __fmaf_rn(p.sum, ot_exp(p.m - a.m), a.sum);
}

// L = m + log(sum); -inf for the empty state
__host__ __device__ __forceinline__ float ot_lse_value(OtLse a) { return a.sum > 0.f ? a.m + logf(a.sum) : -INFINITY; }

// ---- selection: (t, j) as one word whose unsigned order is (t descending, j ascending), for finite t and j >= 0.  The high word of a
// float with bits b is b itself for a negative t and b ^ 0x7FFFFFFF for a positive one (-0 is made +0 first: equal t, equal word);
// the map is its own inverse.  From +FLT_MAX down to -FLT_MAX the high word runs from 0x00800000 up to 0xFF7FFFFF.
constexpr knn_key_t OT_EMPTY = 0xFF800000FFFFFFFFull;   // (-inf, -1): an empty slot, after every key that can be made
__host__ __device__ __forceinline__ unsigned ot_flip(unsigned b) { return (b >> 31) ? b : b ^ 0x7FFFFFFFu; }
__host__ __device__ __forceinline__ knn_key_t ot_key(float t, int j) {
  return ((knn_key_t)ot_flip(__builtin_bit_cast(unsigned, t + 0.f)) << 32) | (knn_key_t)(unsigned)j;
}
__host__ __device__ __forceinline__ float ot_key_t(knn_key_t key) { return __builtin_bit_cast(float, ot_flip((unsigned)(key >> 32))); }
__host__ __device__ __forceinline__ bool ot_key_empty(knn_key_t key) { return key >= 0xFF80000000000000ull; }

// (t, j) goes ahead of the entry `worst`: a t that is not finite never does
__host__ __device__ __forceinline__ bool ot_better(float t, int j, knn_key_t worst) { return ot_finite(t) && ot_key(t, j) < worst; }
__host__ __device__ __forceinline__ void ot_clear(knn_key_t* list, int st, int k) {
  for (int s = 0; s < k; ++s) list[s * st] = OT_EMPTY;
}
__host__ __device__ __forceinline__ void ot_top_init(KnnTop& t) { t.worst = OT_EMPTY; t.wpos = 0; t.fill = 0; }
// ---- OT-CORE-END ----

struct OtArgs {
  const float* Q; long ld_q; int n_q;
  const float* C; long ld_c; int n_c;
  int D, k;
  const float* h;            // [n_c]
  const float* r;            // [n_q] (topk)
  float s;
  int n_split, per;          // chunks, candidates per chunk
  float* L;                  // [n_q] (softmin)
  int* idx; float* val; long ld_out; float* mass;   // (topk)
  void* ws;                  // softmin: [n_split][n_q] OtLse; topk: [n_split][n_q][k] keys (n_split > 1)
};

// the tile and its h, then (topk) the lanes' key slots
constexpr int ot_tile_words(int DP) { return KNN_TC * DP + KNN_TC; }
constexpr int ot_softmin_lds_bytes(int DP) { return ot_tile_words(DP) * 4; }
constexpr int ot_topk_lds_bytes(int DP, int k) { return ot_tile_words(DP) * 4 + (k + KNN_SCAN - 1) / KNN_SCAN * KNN_SCAN * KNN_TQ * 8; }

// pair_scan's staging step: the h of candidates [j0, j0 + n) behind the tile, -inf from n on (such a row's t is never finite).
// `a`: any argument struct with the field h (OtArgs here, OtSegArgs of spv_ot_segments.h)
template <typename Args>
__device__ __forceinline__ void ot_stage_h(const Args& a, float* th, int j0, int n) {
  for (int r = threadIdx.x; r < KNN_TC; r += KNN_TQ) th[r] = r < n ? a.h[j0 + r] : -INFINITY;
}

// grid (query tiles, n_split), KNN_TQ threads, ot_softmin_lds_bytes(DP) of dynamic LDS
template <int DP>
__global__ __launch_bounds__(KNN_TQ) __attribute__((amdgpu_waves_per_eu(2))) void ot_softmin_kernel(const OtArgs a) {
  extern __shared__ __align__(16) float ot_lds[];
  float* const tile = ot_lds;                    // [KNN_TC][DP]
  float* const th = ot_lds + KNN_TC * DP;        // [KNN_TC]
  const int lane = threadIdx.x, i = blockIdx.x * KNN_TQ + lane;
  const bool live = i < a.n_q;

  float q[DP];
  scan_load_query<DP>(a, i, live, q);
  OtLse st;
  ot_lse_init(st);

  pair_scan<DP>(a, q, tile, [&](int j0, int n) { ot_stage_h(a, th, j0, n); },
                [&](int, int row, bool, float c) { ot_update(st, ot_t(c, a.s, th[row])); });   // rows past the chunk's end carry h = -inf: computed, never added
  if (!live) return;
  if (a.n_split == 1) a.L[i] = ot_lse_value(st);
  else reinterpret_cast<OtLse*>(a.ws)[(long)blockIdx.y * a.n_q + i] = st;
}

// grid (query tiles), KNN_TQ threads: the chunks' states in chunk order into one
__global__ __launch_bounds__(KNN_TQ) void ot_softmin_merge_kernel(const OtArgs a) {
  const int i = blockIdx.x * KNN_TQ + threadIdx.x;
  if (i >= a.n_q) return;
  const OtLse* const ws = reinterpret_cast<const OtLse*>(a.ws);
  OtLse st;
  ot_lse_init(st);
  for (int c = 0; c < a.n_split; ++c) ot_merge(st, ws[(long)c * a.n_q + i]);
  a.L[i] = ot_lse_value(st);
}

// a query's sorted keys as its row of idx / val, and the row's mass
__device__ __forceinline__ void ot_write_row(const OtArgs& a, int i, const knn_key_t* list) {
  const long o = (long)i * a.ld_out;
  const float r = a.r[i];
  float mass = 0.f;
  for (int s = 0; s < a.k; ++s) {
    const knn_key_t key = list[s * KNN_TQ];
    const bool none = ot_key_empty(key);
    const float v = none ? 0.f : expf(ot_key_t(key) + r);
    a.idx[o + s] = none ? -1 : knn_key_j(key);
    a.val[o + s] = v;
    mass += v;
  }
  a.mass[i] = mass;
}

// grid (query tiles, n_split), KNN_TQ threads, ot_topk_lds_bytes(DP, k) of dynamic LDS
template <int DP>
__global__ __launch_bounds__(KNN_TQ) __attribute__((amdgpu_waves_per_eu(2))) void ot_topk_kernel(const OtArgs a) {
  extern __shared__ __align__(16) float ot_lds[];
  float* const tile = ot_lds;
  float* const th = ot_lds + KNN_TC * DP;
  knn_key_t* const list = reinterpret_cast<knn_key_t*>(ot_lds + ot_tile_words(DP)) + threadIdx.x;   // [k][KNN_TQ], this lane's column
  const int lane = threadIdx.x, i = blockIdx.x * KNN_TQ + lane, k = a.k;
  const bool live = i < a.n_q;

  float q[DP];
  scan_load_query<DP>(a, i, live, q);
  ot_clear(list, KNN_TQ, k);
  knn_pad(list, KNN_TQ, k);
  KnnTop top;
  ot_top_init(top);

  pair_scan<DP>(a, q, tile, [&](int j0, int n) { ot_stage_h(a, th, j0, n); },
                [&](int j, int row, bool in, float c) {
                  const float t = ot_t(c, a.s, th[row]);
                  if (in && ot_better(t, j, top.worst)) knn_keep(top, list, KNN_TQ, k, ot_key(t, j));
                });
  if (!live) return;
  knn_sort(list, KNN_TQ, top.fill);
  if (a.n_split == 1) ot_write_row(a, i, list);
  else {
    knn_key_t* const ws = reinterpret_cast<knn_key_t*>(a.ws) + ((long)blockIdx.y * a.n_q + i) * k;
    for (int s = 0; s < k; ++s) ws[s] = list[s * KNN_TQ];
  }
}

// grid (query tiles), KNN_TQ threads, k * KNN_TQ * 8 bytes of dynamic LDS: the chunks' lists in chunk order into one list
__global__ __launch_bounds__(KNN_TQ) void ot_topk_merge_kernel(const OtArgs a) {
  extern __shared__ __align__(16) float ot_lds[];
  const int i = blockIdx.x * KNN_TQ + threadIdx.x, k = a.k;
  if (i >= a.n_q) return;
  knn_key_t* const list = reinterpret_cast<knn_key_t*>(ot_lds) + threadIdx.x;
  ot_clear(list, KNN_TQ, k);
  const knn_key_t* const ws = reinterpret_cast<const knn_key_t*>(a.ws);
  for (int c = 0; c < a.n_split; ++c) knn_merge(list, KNN_TQ, k, ws + ((long)c * a.n_q + i) * k);
  ot_write_row(a, i, list);
}

}  // namespace spv
