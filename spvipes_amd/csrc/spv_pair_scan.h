// The all-pairs scan the k-NN, transport and silhouette kernels share (knn_partial_kernel, ot_softmin_kernel, ot_topk_kernel,
// sil_partial_kernel): every query of a workgroup meets every candidate of the workgroup's chunk once, in ascending candidate order,
// with the pair's squared distance as one fixed fp32 chain (knn_step).  What a kernel does with (candidate, distance) is its own.
//
// How the work is laid out on the chip
//   * One query per lane, its vector in DP registers (D padded with zeros to DP = 16 / 32 / 64: fmaf(0, 0, acc) == acc).  A workgroup
//     is KNN_TQ = 128 queries (2 waves) and one chunk of the candidates; the grid is (query tiles) x (chunks): chunk blockIdx.y owns the
//     candidates [blockIdx.y * per, min((blockIdx.y + 1) * per, n_c)), possibly none (knn_chunk).
//   * The chunk passes through LDS KNN_TC = 64 candidates at a time, [candidate][DP] fp32 with the padding and the rows past the chunk's
//     end written as zeros.  All lanes read the same address (a broadcast, no bank conflicts), 16 bytes per read.  Four candidates (two
//     at DP = 64: CAND x DP tile words are in flight next to the DP of the query) are in flight per lane so that independent
//     subtract-fma chains cover the VALU latency at 4 to 12 waves per CU.
// The code here knows nothing of its callers: `a` is any argument struct with the fields C, ld_c, n_c, D and per (Q, ld_q for the query),
// and what differs per kernel comes in as two callables.  Included by spv_knn.h behind its KNN-CORE text, whose constants and knn_step it uses.
#pragma once

namespace spv {

// query i into registers: zeros from D on, and for a lane without a query (!live)
template <int DP, typename Args>
__device__ __forceinline__ void scan_load_query(const Args& a, long i, bool live, float (&q)[DP]) {
#pragma unroll
  for (int t = 0; t < DP; ++t) q[t] = (live && t < a.D) ? a.Q[i * a.ld_q + t] : 0.f;
}

// The scan of this workgroup's chunk.  `tile`: KNN_TC * DP floats of LDS.  Per tile of candidates [j0, j0 + n):
//   stage(j0, n)             between the tile's load and the barrier behind it: whatever else the kernel keeps in LDS per candidate
//   visit(j, row, in, d2)    per candidate j = j0 + row, ascending; `in`: row < n.  A round of CAND candidates is computed whole, so
//                            rows n .. of a last, partly filled round are offered too (zeros: in == false), and no others.
template <int DP, typename Args, typename Stage, typename Visit>
__device__ __forceinline__ void pair_scan(const Args& a, const float (&q)[DP], float* tile, Stage stage, Visit visit) {
  constexpr int CAND = DP > 32 ? KNN_CAND / 2 : KNN_CAND;
  const long first = (long)blockIdx.y * a.per;
  const int c0 = first < a.n_c ? (int)first : a.n_c;
  const int c1 = first + a.per < a.n_c ? (int)(first + a.per) : a.n_c;
  for (int j0 = c0; j0 < c1; j0 += KNN_TC) {
    const int n = c1 - j0 < KNN_TC ? c1 - j0 : KNN_TC;
    __syncthreads();   // the previous tile has been read by every lane
    for (int e = threadIdx.x; e < KNN_TC * DP; e += KNN_TQ) {
      const int r = e / DP, t = e % DP;
      tile[e] = (r < n && t < a.D) ? a.C[(long)(j0 + r) * a.ld_c + t] : 0.f;
    }
    stage(j0, n);
    __syncthreads();
    for (int r = 0; r < n; r += CAND) {
      float acc[CAND];
#pragma unroll
      for (int u = 0; u < CAND; ++u) acc[u] = 0.f;
#pragma unroll
      for (int t = 0; t < DP; t += 4) {
#pragma unroll
        for (int u = 0; u < CAND; ++u) {
          const f4v c = *reinterpret_cast<const f4v*>(tile + (r + u) * DP + t);
          acc[u] = knn_step(acc[u], q[t + 0], c[0]);
          acc[u] = knn_step(acc[u], q[t + 1], c[1]);
          acc[u] = knn_step(acc[u], q[t + 2], c[2]);
          acc[u] = knn_step(acc[u], q[t + 3], c[3]);
        }
      }
#pragma unroll
      for (int u = 0; u < CAND; ++u) visit(j0 + r + u, r + u, r + u < n, acc[u]);
    }
  }
}
// the same for a kernel that stages nothing of its own
template <int DP, typename Args, typename Visit>
__device__ __forceinline__ void pair_scan(const Args& a, const float (&q)[DP], float* tile, Visit visit) {
  pair_scan<DP>(a, q, tile, [](int, int) {}, visit);
}

}  // namespace spv
