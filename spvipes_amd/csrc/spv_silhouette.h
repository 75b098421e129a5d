// Segmented distance sums in a low-dimensional space (spv_silhouette_sums; spVIPES.latent_silhouette / integration_scores of the user
// API): for every query row and every SEGMENT of the candidates the fp64 sum of the Euclidean distances to the segment's rows, nothing
// of size queries x candidates ever stored.  The exact silhouette width of a cell is two divisions and a minimum over such sums.
//
//   S[s][i] = sum over j in [seg_ptr[s], seg_ptr[s + 1]) of (double) d(i, j),     d(i, j) = fl32(sqrt(d2(i, j)))
//
// d2 is knn_d2 of spv_knn.h, the fixed fp32 subtract-and-fma chain: bit for bit the squared distance latent_neighbors reports, so a
// query that is also a candidate adds d = +0 for itself and the caller needs no exclusion list.  The root is sqrtf, which the build's
// flags compile to v_sqrt_f32 plus the two-neighbour fma correction: correctly rounded (the bare 1-ulp instruction is what __fsqrt_rn
// gives here, not this).
//
// How the work is laid out on the chip: pair_scan of spv_pair_scan.h, which states the layout (one query per lane, the grid
// (query tiles) x (chunks), the chunk through LDS a tile at a time), with this reduction.  The chunk count is a knn_splits-style pure
// function of the shapes (sil_splits).
//   * The candidates come ARRANGED BY SEGMENT, so each lane keeps ONE fp64 accumulator: a segment's end is the same candidate for
//     every lane, a uniform (scalar) compare and branch per candidate.  At a boundary the lane writes its accumulator to its column of S
//     and clears it (sil_advance); per candidate it pays the DP-term chain, one sqrtf, one convert and one fp64 add (sil_add).  Bins
//     per segment in LDS with a read-modify-write per candidate are what the arrangement makes unnecessary.
//   * S is [segment][query]: at a boundary the 128 lanes of a workgroup write 128 consecutive doubles.
//   * n_split > 1: every (query tile, chunk) writes ALL n_seg sums of its chunk -- zeros for the segments the chunk does not reach --
//     into the workspace [chunk][segment][query], and sil_merge_kernel, one lane per (query, segment), adds the chunks' values in
//     chunk order from +0.  n_split == 1 writes S directly: one launch.
// Order of addition: ascending candidate within a chunk, ascending chunk across chunks, no floating-point atomics.  For fixed shapes and
// n_split two calls agree bit for bit, and a query's sums do not depend on the other queries of the call (its lane sees its own vector
// and the candidates, nothing else).  Different n_split may differ in the last bits of fp64 -- a sum's grouping changes its rounding --
// except where every partial sum is exact (the sum fits in 53 bits at the last place of its smallest term), where they cannot.
// Non-finite inputs: a candidate row with a NaN or an infinity makes the sums of ITS segment NaN / inf for every query, a query row
// with one makes all of its own sums so; nothing else changes.  An empty segment gives +0.
// A seg_ptr that is not ascending from 0 to n_c gives unspecified sums, never an access outside seg_ptr[0 .. n_seg], S or ws.
//
// Registers and occupancy of the three DP forms: the table at sil_partial_kernel (96 / 176 / 208 VGPRs, no scratch).
//
// The part between the two SIL-CORE marks is plain C++ apart from __host__ __device__: tools/silhouette_host_check.py compiles exactly
// that text, after the KNN-CORE text it builds on, for the CPU.
#pragma once
#include "spv_knn.h"

namespace spv {

// ---- SIL-CORE-BEGIN ----
constexpr int SIL_SEG_MAX = 256;   // SPV_SILHOUETTE_SEG_MAX

// the distance of one pair from its squared distance: the correctly rounded fp32 root
__host__ __device__ __forceinline__ float sil_root(float d2) { return sqrtf(d2); }

// a lane's walk over its chunk: the sum of the current segment `s`, which ends ahead of candidate `end`
struct SilWalk { double sum; int s, end; };
__host__ __device__ __forceinline__ void sil_walk_init(SilWalk& w, const int* seg_ptr) { w.sum = 0.0; w.s = 0; w.end = seg_ptr[1]; }

// ahead of candidate j: every segment that ends at or before j is written (`out` is the lane's column, `st` its stride; `write`: the
// lane has a query) and left.  s never passes n_seg - 1, whatever seg_ptr holds.
__host__ __device__ __forceinline__ void sil_advance(SilWalk& w, int j, const int* seg_ptr, int n_seg, double* out, long st, bool write) {
  while (j >= w.end && w.s < n_seg - 1) {
    if (write) out[w.s * st] = w.sum;
    w.sum = 0.0;
    ++w.s;
    w.end = seg_ptr[w.s + 1];
  }
}

// candidate j's squared distance joins the current segment's sum
__host__ __device__ __forceinline__ void sil_add(SilWalk& w, float d2) { w.sum += (double)sil_root(d2); }

// after the chunk's last candidate: the current segment's sum, then +0 for every later segment
__host__ __device__ __forceinline__ void sil_finish(SilWalk& w, int n_seg, double* out, long st, bool write) {
  for (; w.s < n_seg; ++w.s) {
    if (write) out[w.s * st] = w.sum;
    w.sum = 0.0;
  }
}

// the chunks' partial sums of one (segment, query), `st` apart, added in chunk order from +0
__host__ __device__ __forceinline__ double sil_merge(const double* part, long st, int n_split) {
  double sum = 0.0;
  for (int c = 0; c < n_split; ++c) sum += part[c * st];
  return sum;
}

// chunks of the candidates = workgroups per query tile; a pure function of the shapes.  The scan has no per-chunk state beyond one
// double per segment, so chunks are cheap and the plan aims at SIL_TARGET_WG workgroups: several rounds of the 1024 (DP 32 / 64) or
// 2560 (DP 16) that are resident at a time, which keeps the last, partly filled round short against the whole (the k-NN scan's 1024
// left 1173 workgroups at 50 000 x 50 000: a full round and a round of 149).
constexpr int SIL_TARGET_WG = 5120;
inline int sil_splits(int n_q, int n_c) {
  if (n_q < 1 || n_c < 1) return 1;
  const long long tiles = ((long long)n_q + KNN_TQ - 1) / KNN_TQ;
  if (tiles >= SIL_TARGET_WG) return 1;
  int s = (int)((SIL_TARGET_WG + tiles - 1) / tiles);
  const int most = n_c / (KNN_MIN_TILES * KNN_TC);
  if (s > most) s = most;
  if (s > KNN_SPLIT_MAX) s = KNN_SPLIT_MAX;
  return s < 1 ? 1 : s;
}

// bytes of [n_split][n_seg][n_q] doubles; 0 for one chunk or a non-positive shape
inline long long sil_ws_bytes(int n_q, int n_seg, int n_split) {
  if (n_q < 1 || n_seg < 1 || n_split <= 1) return 0;
  return (long long)n_split * n_seg * n_q * 8;
}
// ---- SIL-CORE-END ----

struct SilArgs {
  const float* Q; long ld_q; int n_q;
  const float* C; long ld_c; int n_c;
  int D;
  const int* seg_ptr; int n_seg;
  int n_split, per;          // chunks, candidates per chunk
  double* S; long ld_s;      // [n_seg][ld_s]
  double* ws;                // [n_split][n_seg][n_q] (n_split > 1)
};

constexpr int sil_lds_bytes(int DP) { return KNN_TC * DP * 4; }

// grid (query tiles, n_split), KNN_TQ threads, sil_lds_bytes(DP) of dynamic LDS (4 / 8 / 16 KiB).
//   DP   VGPRs   SGPRs   scratch   waves per SIMD   workgroups per CU (2 waves each; the LDS would allow 10 and more)
//   16     96      38       0           5                10
//   32    176      38       0           2                 4
//   64    208      38       0           2                 4
// (what the compiler reports for this text with the build's flags: the k-NN scan's figures, the fp64 accumulator and the root's
// temporaries fit into what the tile reads in flight already take.  The root is v_sqrt_f32 with the two-neighbour fma correction
// and the denormal scaling around it; the boundary test is s_cmp / s_cbranch.  The attribute keeps any later form from going past 256.)
template <int DP>
__global__ __launch_bounds__(KNN_TQ) __attribute__((amdgpu_waves_per_eu(2))) void sil_partial_kernel(const SilArgs a) {
  extern __shared__ __align__(16) float sil_lds[];
  float* const tile = sil_lds;   // [KNN_TC][DP]
  const int lane = threadIdx.x;
  const long i = (long)blockIdx.x * KNN_TQ + lane;
  const bool live = i < a.n_q;

  float q[DP];
  scan_load_query<DP>(a, i, live, q);

  // this lane's column: of S itself, or of this chunk's slab of the workspace
  const long st = a.n_split == 1 ? a.ld_s : (long)a.n_q;
  double* const out = (a.n_split == 1 ? a.S : a.ws + (long)blockIdx.y * a.n_seg * a.n_q) + (live ? i : 0);
  SilWalk w;
  sil_walk_init(w, a.seg_ptr);

  pair_scan<DP>(a, q, tile, [&](int j, int, bool in, float d2) {   // rows past the chunk's end: computed, never added
    if (in) {   // the same for every lane, as are the boundaries
      sil_advance(w, j, a.seg_ptr, a.n_seg, out, st, live);
      sil_add(w, d2);
    }
  });
  sil_finish(w, a.n_seg, out, st, live);
}

// grid (query tiles, n_seg), KNN_TQ threads: the chunks' sums of one (segment, query) in chunk order into S
__global__ __launch_bounds__(KNN_TQ) void sil_merge_kernel(const SilArgs a) {
  const long i = (long)blockIdx.x * KNN_TQ + threadIdx.x;
  const int s = blockIdx.y;
  if (i >= a.n_q) return;
  a.S[s * a.ld_s + i] = sil_merge(a.ws + (long)s * a.n_q + i, (long)a.n_seg * a.n_q, a.n_split);
}

}  // namespace spv
