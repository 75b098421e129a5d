// Barycentric projection through the UNTRUNCATED transport plan (spv_ot_project; spVIPES.transport_project of the user API): for every
// query row the plan-weighted mean of the candidates' value rows, nothing of size queries x candidates ever stored.
//
//   out[v][i] = sum_j exp(t_ij) V[j][v] / sum_j exp(t_ij),     t_ij = ot_t(c_ij, s, h_j),     L[i] = log sum_j exp(t_ij)
//
// t is spv_ot.h's, the same bits as ot_softmin_kernel's: with h = psi + log b of a Sinkhorn result the weights are the row of the plan
// P_ij = a_i b_j exp(phi_i + psi_j - s c_ij) up to the row's own factor, which the quotient drops.  This is attention with a Euclidean
// score: ot_softmin's running (m, sum) pair plus one accumulator per value column, rescaled whenever the running maximum rises.
//
// How the work is laid out on the chip: pair_scan of spv_pair_scan.h, which states the layout (one query per lane, the grid
// (query tiles) x (chunks), the chunk through LDS a tile at a time), times COLUMN BLOCKS of VB value columns on blockIdx.z; every block
// rescans the distances.  Behind the tile and its h (ot_stage_h) the tile's value rows V[j0 .. j0 + n)[v0 .. v0 + VB) are staged,
// [candidate][VB] fp32 with zeros for the rows past the chunk's end and the columns past n_v; all lanes read the same address.
//   * A lane holds an OtLse and acc[VB].  Per candidate with a finite t: d = t - m, e = ot_exp(-|d|); (m, sum) by ot_update itself, and
//     ONE fma per column: acc = fmaf(acc, e, V) where the maximum rises (d > 0), acc = fmaf(e, V, acc) otherwise.  A t that is not finite
//     contributes nothing: its value row never enters a sum, whatever it holds.
//   * QUIET ROUNDS.  A round of CAND candidates in which no lane of the wave meets a new maximum or a t that is not finite (one vote
//     per round) leaves every m where it is: the round's exponentials are independent and its update is straight-line code,
//     otproj_stay, the same operations in the same order as otproj_update's.  Any other round takes otproj_update per candidate.
//     Which route a round takes depends on the other lanes of the wave; the bits do not.
//   * n_split == 1: the lane writes out[v][i] = acc_v / sum (the correctly rounded quotient) and, in column block 0, L[i]: ONE launch.
//   * n_split > 1: every (query tile, chunk, column block) writes (m, sum, acc[0 .. live columns)) to the workspace
//     [chunk][n_v + 2 * blocks][n_q]: block z owns the rows from z * (VB + 2) on, lanes write consecutive words.  otproj_merge_kernel,
//     one lane per (query, column), folds the chunks IN CHUNK ORDER from the empty state by ot_merge's rule extended to acc
//     (otproj_merge).  No floating-point atomics anywhere.
//   * A column's operations do not depend on the other columns of the call: (m, sum) is every block's own copy of the same sequence,
//     and a column of ones repeats the sum's very operations -- its accumulator EQUALS sum and comes back as exactly 1.0f.
//   * The chunk plan for a given n_split is knn_chunk's and (m, sum) takes ot_update / ot_merge: L EQUALS spv_ot_softmin's at the same
//     explicit n_split.  The automatic count (otproj_splits) is knn_splits' plan with the column blocks counted among the workgroups:
//     a chunk's state is n_v + 2 words per query where ot_softmin's is 2, small next to the >= 256 candidates a chunk scans but not
//     free, so the plan aims at KNN_TARGET_WG workgroups (one round of resident ones) like ot_softmin's, not at otseg_splits' several
//     rounds.  It counts blocks of 32 columns whatever D (the count must be a function of (n_q, n_c, n_v) alone).
// What is reproducible: for fixed (shapes, n_split) two calls agree bit for bit; a query's row does not depend on the other queries of
// the call, a column not on the other columns.  Different n_split agree within the bound of tests/test_gpu_ot_project.py only.
// A query without a contributing candidate (n_c = 0 included) gets L = -inf and 0 / 0 = NaN in every column: the mean of nothing.
//
// Registers of the three DP forms and the block widths they allow: the table at otproj_partial_kernel.
//
// The part between the two OTPROJ-CORE marks is plain C++ apart from __host__ __device__ and the rounding intrinsics:
// tools/ot_project_host_check.py compiles exactly that text, after the KNN-CORE and OT-CORE texts it builds on, for the CPU.
#pragma once
#include "spv_ot.h"

namespace spv {

// ---- OTPROJ-CORE-BEGIN ----
constexpr int OT_VAL_MAX = 256;   // SPV_OT_VAL_MAX
// value columns per column block (acc registers per lane) of the DP 16 / 32 / 64 forms
constexpr int otproj_block(int DP) { return DP > 32 ? 16 : 32; }
constexpr int OT_PROJ_VB_MIN = 16, OT_PROJ_VB_MAX = 32;

// a lane's state: the log-sum-exp pair and sum_j exp(t_j - m) V[j][v] per column; ((-inf, 0), zeros) before the first term
template <int VB>
struct OtProj { OtLse st; float acc[VB]; };
template <int VB>
__host__ __device__ __forceinline__ void otproj_init(OtProj<VB>& a) {
  ot_lse_init(a.st);
  for (int v = 0; v < VB; ++v) a.acc[v] = 0.f;
}

// one more term with the value row `val` [VB].  The first finite t meets m = -inf: e = 0, acc = fma(0, 0, V) = V next to sum = 1.
template <int VB>
__host__ __device__ __forceinline__ void otproj_update(OtProj<VB>& a, float t, const float* val) {
  if (!ot_finite(t)) return;
  const float d = t - a.st.m;
  const float e = ot_exp(-fabsf(d));
  if (d > 0.f) {
    for (int v = 0; v < VB; ++v) a.acc[v] = __fmaf_rn(a.acc[v], e, val[v]);
  } else {
    for (int v = 0; v < VB; ++v) a.acc[v] = __fmaf_rn(e, val[v], a.acc[v]);
  }
  ot_update(a.st, t);   // the same d and e
}

// t is finite and does not exceed the running maximum: otproj_update would take neither its return nor its rescale branch
template <int VB>
__host__ __device__ __forceinline__ bool otproj_stays(const OtProj<VB>& a, float t) { return ot_finite(t) && !(t - a.st.m > 0.f); }

// otproj_update for a t that otproj_stays: the same operations in the same order, without a test.  m does not change, so a run of
// such terms may be tested against the state ahead of the run and then added one after the other (the kernel's quiet rounds).
template <int VB>
__host__ __device__ __forceinline__ void otproj_stay(OtProj<VB>& a, float t, const float* val) {
  const float d = t - a.st.m;
  const float e = ot_exp(-fabsf(d));
  for (int v = 0; v < VB; ++v) a.acc[v] = __fmaf_rn(e, val[v], a.acc[v]);
  a.st.sum += e;
}

// the state of a later chunk joins: ot_merge, and its rule for the n accumulators `acc` (stride 1) and the chunk's `pacc`, `stride` apart
__host__ __device__ __forceinline__ void otproj_merge(OtLse& a, float* acc, int n, OtLse p, const float* pacc, long stride) {
  if (p.m > a.m) {
    const float e = ot_exp(a.m - p.m);
    for (int v = 0; v < n; ++v) acc[v] = __fmaf_rn(acc[v], e, pacc[v * stride]);
  } else if (p.sum > 0.f) {
    const float e = ot_exp(p.m - a.m);
    for (int v = 0; v < n; ++v) acc[v] = __fmaf_rn(pacc[v * stride], e, acc[v]);
  }
  ot_merge(a, p);
}

// the weighted mean of a column: the correctly rounded quotient; 0 / 0 = NaN for the empty state
__host__ __device__ __forceinline__ float otproj_value(float acc, OtLse st) { return __fdiv_rn(acc, st.sum); }

// the workspace [chunk][otproj_ws_rows][n_q]: column block z owns the rows from z * (VB + 2) on -- m, sum, then its live columns --
// which is row v + 2 * (v / VB + 1) for column v
__host__ __device__ __forceinline__ int otproj_ws_rows(int n_v, int VB) { return n_v + 2 * ((n_v + VB - 1) / VB); }

// chunks of the candidates: knn_splits' plan with the column blocks (of OT_PROJ_VB_MAX columns, whatever D) counted among the workgroups
inline int otproj_splits(int n_q, int n_c, int n_v) {
  if (n_q < 1 || n_c < 1 || n_v < 1) return 1;
  const long long wg = (((long long)n_q + KNN_TQ - 1) / KNN_TQ) * (((long long)n_v + OT_PROJ_VB_MAX - 1) / OT_PROJ_VB_MAX);
  if (2 * wg >= KNN_TARGET_WG) return 1;
  int s = (int)((KNN_TARGET_WG + wg - 1) / wg);
  const int most = n_c / (KNN_MIN_TILES * KNN_TC);
  if (s > most) s = most;
  if (s > KNN_SPLIT_MAX) s = KNN_SPLIT_MAX;
  return s < 1 ? 1 : s;
}

// fp32 words per (chunk, query) at the narrowest block width, which has the most (m, sum) rows: enough for every D
inline long long otproj_ws_words(int n_q, int n_v, int n_split) {
  if (n_q < 1 || n_v < 1 || n_split <= 1) return 0;
  return (long long)n_split * otproj_ws_rows(n_v, OT_PROJ_VB_MIN) * n_q;
}
inline long long otproj_ws_bytes(int n_q, int n_v, int n_split) { return otproj_ws_words(n_q, n_v, n_split) * 4; }
// ---- OTPROJ-CORE-END ----

struct OtProjArgs {
  const float* Q; long ld_q; int n_q;
  const float* C; long ld_c; int n_c;
  int D;
  const float* h;            // [n_c]
  float s;
  const float* V; long ld_v; int n_v;   // [n_c][ld_v]
  int n_split, per;          // chunks, candidates per chunk
  float* out; long ld_out;   // [n_v][ld_out]
  float* L;                  // [n_q] or null
  float* ws;                 // [n_split][ws_rows][n_q] (n_split > 1)
  int ws_rows;               // otproj_ws_rows(n_v, VB of this D)
};

constexpr int otproj_lds_bytes(int DP) { return (ot_tile_words(DP) + KNN_TC * otproj_block(DP)) * 4; }

// grid (query tiles, n_split, column blocks), KNN_TQ threads, otproj_lds_bytes(DP) of dynamic LDS (the tile, its h, its value rows).
//   DP   VB   VGPRs   SGPRs   scratch   waves per SIMD   workgroups per CU (2 waves each)
//   16   32    150      54       0           3                 6
//   32   32    176      54       0           2                 4
//   64   16    239      50       0           2                 4
// (what the compiler reports for this text with the build's flags.  ot_softmin_kernel's figures are 80 / 144 / 144 VGPRs: the
// accumulators add VB, the rest is the value rows of a quiet round in flight -- CAND x VB words, which the scheduler trims to what
// the attribute's 256 registers leave.  DP 64, whose query alone holds 64 registers, takes 16 columns.  A first form without the
// quiet rounds -- otproj_update per candidate, its value row read behind the update's branches -- stood at 162 / 222 / 190 VGPRs
// and ran 1.2 to 1.4 times as long at DP 16 / 32: DESIGN.md section 23 has both forms' measured times.)
template <int DP>
__global__ __launch_bounds__(KNN_TQ) __attribute__((amdgpu_waves_per_eu(2))) void otproj_partial_kernel(const OtProjArgs a) {
  constexpr int VB = otproj_block(DP);
  extern __shared__ __align__(16) float otproj_lds[];
  float* const tile = otproj_lds;                      // [KNN_TC][DP]
  float* const th = otproj_lds + KNN_TC * DP;          // [KNN_TC]
  float* const tv = otproj_lds + ot_tile_words(DP);    // [KNN_TC][VB]
  const int lane = threadIdx.x, v0 = blockIdx.z * VB;
  const int n_col = a.n_v - v0 < VB ? a.n_v - v0 : VB;   // this block's live columns, >= 1
  const long i = (long)blockIdx.x * KNN_TQ + lane;
  const bool live = i < a.n_q;

  float q[DP];
  scan_load_query<DP>(a, i, live, q);
  OtProj<VB> st;
  otproj_init(st);

  // pair_scan offers the candidates in rounds of CAND (its own constant, restated), the round's first at a row that is a multiple of
  // CAND.  The round's t are collected and the round is taken at its last candidate.  A round in which no lane of the wave meets a t
  // that is not finite or a new maximum is `quiet`: m stands still, the CAND exponentials are independent, and the update is
  // straight-line code -- CAND x VB fmas per lane with the value rows as 16-byte broadcast reads ahead of them, no branch for the
  // reads to wait behind.  Any other round (the first of a chunk, a rise in some lane, rows past the chunk's end, which carry
  // h = -inf) takes otproj_update candidate by candidate.  Both routes perform the same operations in the same order.
  constexpr int CAND = DP > 32 ? KNN_CAND / 2 : KNN_CAND;
  float tr[CAND];
#pragma unroll
  for (int u = 0; u < CAND; ++u) tr[u] = -INFINITY;
  pair_scan<DP>(a, q, tile,
                [&](int j0, int n) {
                  ot_stage_h(a, th, j0, n);
                  for (int e = threadIdx.x; e < KNN_TC * VB; e += KNN_TQ) {
                    const int r = e / VB, c = e % VB;
                    tv[e] = (r < n && c < n_col) ? a.V[(long)(j0 + r) * a.ld_v + v0 + c] : 0.f;
                  }
                },
                [&](int, int row, bool, float c) {
#pragma unroll
                  for (int u = 0; u + 1 < CAND; ++u) tr[u] = tr[u + 1];
                  tr[CAND - 1] = ot_t(c, a.s, th[row]);
                  if ((row & (CAND - 1)) != CAND - 1) return;   // the same for every lane
                  const float* const rows = tv + (row - (CAND - 1)) * VB;
                  bool quiet = true;
#pragma unroll
                  for (int u = 0; u < CAND; ++u) quiet = quiet && otproj_stays(st, tr[u]);
                  if (__all(quiet)) {
#pragma unroll
                    for (int u = 0; u < CAND; ++u) {
                      float val[VB];
#pragma unroll
                      for (int v = 0; v < VB; v += 4) {
                        const f4v x = *reinterpret_cast<const f4v*>(rows + u * VB + v);
                        val[v] = x[0], val[v + 1] = x[1], val[v + 2] = x[2], val[v + 3] = x[3];
                      }
                      otproj_stay(st, tr[u], val);
                    }
                  } else {
#pragma unroll
                    for (int u = 0; u < CAND; ++u) otproj_update(st, tr[u], rows + u * VB);
                  }
                });
  if (!live) return;
  if (a.n_split == 1) {
#pragma unroll
    for (int c = 0; c < VB; ++c)
      if (c < n_col) a.out[(long)(v0 + c) * a.ld_out + i] = otproj_value(st.acc[c], st.st);
    if (blockIdx.z == 0 && a.L) a.L[i] = ot_lse_value(st.st);
  } else {
    float* const w = a.ws + ((long)blockIdx.y * a.ws_rows + (long)blockIdx.z * (VB + 2)) * a.n_q + i;
    w[0] = st.st.m;
    w[a.n_q] = st.st.sum;
#pragma unroll
    for (int c = 0; c < VB; ++c)
      if (c < n_col) w[(long)(2 + c) * a.n_q] = st.acc[c];
  }
}

// grid (query tiles, n_v), KNN_TQ threads: the chunks' states of one (query, column) in chunk order into out, and into L next to column 0.
// `VB`: the block width the partial pass ran with
__global__ __launch_bounds__(KNN_TQ) void otproj_merge_kernel(const OtProjArgs a, int VB) {
  const long i = (long)blockIdx.x * KNN_TQ + threadIdx.x;
  const int v = blockIdx.y, z = v / VB;
  if (i >= a.n_q) return;
  const float* const w = a.ws + (long)z * (VB + 2) * a.n_q + i;   // the block's m; its sum one row on, column v at row 2 + v - z * VB
  const long chunk = (long)a.ws_rows * a.n_q, col = (long)(2 + v - z * VB) * a.n_q;
  OtLse st;
  ot_lse_init(st);
  float acc = 0.f;
  for (int c = 0; c < a.n_split; ++c) otproj_merge(st, &acc, 1, OtLse{w[c * chunk], w[c * chunk + a.n_q]}, w + c * chunk + col, 0);
  a.out[(long)v * a.ld_out + i] = otproj_value(acc, st);
  if (v == 0 && a.L) a.L[i] = ot_lse_value(st);
}

}  // namespace spv
