// Segmented log-sum-exp of the transport kernel (spv_ot_segment_lse; spVIPES.match_transport_clusters of the user API): for every query
// row and every SEGMENT of the candidates the log of the plan's mass between the query and the segment, up to the query's own
// potential, nothing of size queries x candidates ever stored.
//
//   L[s][i] = log sum over j in [seg_ptr[s], seg_ptr[s + 1]) of exp(t_ij),     t_ij = ot_t(c_ij, s, h_j)
//
// t is spv_ot.h's, the same bits as ot_softmin_kernel's and ot_topk_kernel's: with h = psi + log b of a Sinkhorn result and
// r_i = phi_i + log a_i, exp(L[s][i] + r_i) is the mass the UNTRUNCATED plan P_ij = exp(t_ij + r_i) puts between cell i and the cells
// of segment s.  The stored plan keeps k entries per cell; its segment sums are biased towards each cell's nearest partners.
//
// How the work is laid out on the chip: pair_scan of spv_pair_scan.h, which states the layout (one query per lane, the grid
// (query tiles) x (chunks), the chunk through LDS a tile at a time), the tile's h staged behind the tile by ot_stage_h, and
// spv_silhouette.h's walk over segments with spv_ot.h's running (m, sum) pair as the one accumulator of a lane:
//   * The candidates come ARRANGED BY SEGMENT: a segment's end is the same candidate for every lane, a uniform (scalar) compare and
//     branch.  At a boundary the lane writes its state and re-initialises it (otseg_advance); per candidate it pays the DP-term
//     chain, one fma and ot_update's one exp (otseg_add).  The compare is made once per ROUND of candidates (otseg_quiet): a round
//     inside one segment runs without a test per candidate.
//   * n_split == 1: the lane writes ot_lse_value(state) into L, fp32 [segment][ld_l]: the 128 lanes of a workgroup write 128
//     consecutive floats.  ONE launch.
//   * n_split > 1: every (query tile, chunk) writes ALL n_seg states of its chunk -- the empty state (-inf, 0) for the segments the
//     chunk does not reach -- into the workspace [chunk][segment][query], and otseg_merge_kernel, one lane per (query, segment), folds
//     them with ot_merge IN CHUNK ORDER from the empty state and takes ot_lse_value.  No floating-point atomics anywhere.
//   * The chunk plan for a given n_split is knn_chunk's, as ot_softmin_kernel's.  With n_seg == 1 the walk never meets a boundary and
//     the lane performs ot_softmin_kernel's very sequence of operations: L[0] EQUALS spv_ot_softmin's L at the same explicit n_split.
//     The automatic chunk count (otseg_splits) is sil_splits' plan, not knn_splits': the per-chunk state is 8 bytes per segment, so
//     chunks are cheap and several rounds of resident workgroups keep the last, partly filled round short.
// What is reproducible: for fixed (shapes, n_split) two calls agree bit for bit; a query's values do not depend on the other queries of
// the call.  Different n_split agree within the bound of tests/test_gpu_ot_segments.py (spv_ot_softmin's), not bit for bit.
// A t that is not finite contributes nothing (a NaN row, h = -inf, a cost that overflowed); a segment without a contributing candidate
// gives -inf: an empty segment, n_c = 0.  A seg_ptr that is not ascending from 0 to n_c gives unspecified values, never an access
// outside seg_ptr[0 .. n_seg], L or ws: the walk reads seg_ptr[s + 1] for s <= n_seg - 1 only and writes slots 0 .. n_seg - 1 only.
//
// Registers of the three DP forms: the table at otseg_partial_kernel (89 / 153 / 153 VGPRs, no scratch: ot_softmin_kernel's occupancy
// class at DP 32 / 64, one wave short of it at DP 16; the table says what it took).
//
// The part between the two OTSEG-CORE marks is plain C++ apart from __host__ __device__: tools/ot_segment_host_check.py compiles
// exactly that text, after the KNN-CORE and OT-CORE texts it builds on, for the CPU.
#pragma once
#include "spv_ot.h"

namespace spv {

// ---- OTSEG-CORE-BEGIN ----
constexpr int OT_SEG_MAX = 256;   // SPV_OT_SEG_MAX

// a lane's walk over its chunk: the state of the current segment `s`, which ends ahead of candidate `end`
struct OtSegWalk { OtLse st; int s, end; };
__host__ __device__ __forceinline__ void otseg_walk_init(OtSegWalk& w, const int* seg_ptr) { ot_lse_init(w.st); w.s = 0; w.end = seg_ptr[1]; }

// a lane's column of the output: of L itself (one chunk: the finished value) or of its chunk's slab of the workspace (the state).
// Exactly one of the two pointers is set; `stride`: floats / states between two segments
struct OtSegOut { float* L; OtLse* ws; long stride; };
__host__ __device__ __forceinline__ void otseg_write(const OtSegOut& o, int s, OtLse st) {
  if (o.L) o.L[s * o.stride] = ot_lse_value(st);
  else o.ws[s * o.stride] = st;
}

// ahead of candidate j: every segment that ends at or before j is written (`write`: the lane has a query) and left, the state
// re-initialised.  s never passes n_seg - 1, whatever seg_ptr holds.
__host__ __device__ __forceinline__ void otseg_advance(OtSegWalk& w, int j, const int* seg_ptr, int n_seg, const OtSegOut& o, bool write) {
  while (j >= w.end && w.s < n_seg - 1) {
    if (write) otseg_write(o, w.s, w.st);
    ot_lse_init(w.st);
    ++w.s;
    w.end = seg_ptr[w.s + 1];
  }
}

// the candidates [j, j + cand) all belong to the current segment: none of them needs otseg_advance.  (Ahead of candidate j the walk
// stands in j's segment or before it; j + cand <= end > j says it is j's, and the others' too.)
__host__ __device__ __forceinline__ bool otseg_quiet(const OtSegWalk& w, int j, int cand) { return j + cand <= w.end; }

// candidate j's t joins the current segment's state: ot_softmin_kernel's step
__host__ __device__ __forceinline__ void otseg_add(OtSegWalk& w, float t) { ot_update(w.st, t); }

// after the chunk's last candidate: the current segment's state, then the empty state for every later segment
__host__ __device__ __forceinline__ void otseg_finish(OtSegWalk& w, int n_seg, const OtSegOut& o, bool write) {
  for (; w.s < n_seg; ++w.s) {
    if (write) otseg_write(o, w.s, w.st);
    ot_lse_init(w.st);
  }
}

// the chunks' states of one (segment, query), `stride` apart, folded in chunk order from the empty state: ot_softmin_merge_kernel's loop
__host__ __device__ __forceinline__ float otseg_merge(const OtLse* part, long stride, int n_split) {
  OtLse st;
  ot_lse_init(st);
  for (int c = 0; c < n_split; ++c) ot_merge(st, part[c * stride]);
  return ot_lse_value(st);
}

// chunks of the candidates = workgroups per query tile; a pure function of the shapes.  A chunk's state is one (m, sum) pair per
// segment, so chunks are cheap and the plan aims at OT_SEG_TARGET_WG workgroups: several rounds of the 1024 (DP 32 / 64) or 2560
// (DP 16) that are resident at a time (the silhouette scan's plan and reasoning: spv_silhouette.h, sil_splits).
constexpr int OT_SEG_TARGET_WG = 5120;
inline int otseg_splits(int n_q, int n_c) {
  if (n_q < 1 || n_c < 1) return 1;
  const long long tiles = ((long long)n_q + KNN_TQ - 1) / KNN_TQ;
  if (tiles >= OT_SEG_TARGET_WG) return 1;
  int s = (int)((OT_SEG_TARGET_WG + tiles - 1) / tiles);
  const int most = n_c / (KNN_MIN_TILES * KNN_TC);
  if (s > most) s = most;
  if (s > KNN_SPLIT_MAX) s = KNN_SPLIT_MAX;
  return s < 1 ? 1 : s;
}

// bytes of [n_split][n_seg][n_q] states; 0 for one chunk or a non-positive shape
inline long long otseg_ws_bytes(int n_q, int n_seg, int n_split) {
  if (n_q < 1 || n_seg < 1 || n_split <= 1) return 0;
  return (long long)n_split * n_seg * n_q * (long long)sizeof(OtLse);
}
// ---- OTSEG-CORE-END ----

struct OtSegArgs {
  const float* Q; long ld_q; int n_q;
  const float* C; long ld_c; int n_c;
  int D;
  const float* h;            // [n_c]
  float s;
  const int* seg_ptr; int n_seg;
  int n_split, per;          // chunks, candidates per chunk
  float* L; long ld_l;       // [n_seg][ld_l]
  OtLse* ws;                 // [n_split][n_seg][n_q] (n_split > 1)
};

// grid (query tiles, n_split), KNN_TQ threads, ot_softmin_lds_bytes(DP) of dynamic LDS (the tile and its h).
//   DP   VGPRs   SGPRs   scratch   waves per SIMD   workgroups per CU (2 waves each)
//   16     89      63       0           5                10
//   32    153      63       0           3                 6
//   64    153      62       0           3                 6
// (what the compiler reports for this text with the build's flags.  ot_softmin_kernel's figures are 80 / 144 / 144 VGPRs, 6 / 3 / 3
// waves: the DP 32 / 64 forms keep its class, the DP 16 form is one wave short of it.  What makes the difference is the round test
// below.  With the boundary test at EVERY candidate -- s_cmp / s_cbranch, a store and a logf behind it -- the figures were 104 / 184 /
// 216 VGPRs and 4 / 2 / 2 waves, sil_partial_kernel's class: the accumulators of a round of candidates and the lane's output addresses
// stayed live across the branches.  A round without a boundary now runs ot_softmin_kernel's straight-line visits.  DESIGN.md section
// 22 has both forms' measured times.  The attribute keeps any later form from going past 256.)
template <int DP>
__global__ __launch_bounds__(KNN_TQ) __attribute__((amdgpu_waves_per_eu(2))) void otseg_partial_kernel(const OtSegArgs a) {
  extern __shared__ __align__(16) float otseg_lds[];
  float* const tile = otseg_lds;                    // [KNN_TC][DP]
  float* const th = otseg_lds + KNN_TC * DP;        // [KNN_TC]
  const int lane = threadIdx.x;
  const long i = (long)blockIdx.x * KNN_TQ + lane;
  const bool live = i < a.n_q;

  float q[DP];
  scan_load_query<DP>(a, i, live, q);

  // this lane's column: of L itself, or of this chunk's slab of the workspace
  const long col = live ? i : 0;
  const OtSegOut out = a.n_split == 1 ? OtSegOut{a.L + col, nullptr, a.ld_l}
                                      : OtSegOut{nullptr, a.ws + (long)blockIdx.y * a.n_seg * a.n_q + col, (long)a.n_q};
  OtSegWalk w;
  otseg_walk_init(w, a.seg_ptr);

  // pair_scan offers the candidates in rounds of CAND (its own constant, restated), the round's first at a row that is a multiple of
  // CAND.  A round that lies inside the current segment is `quiet`: no test and no branch per candidate, ot_softmin_kernel's visit
  // (a row past the chunk's end carries h = -inf and adds nothing).  Any other round takes the walk candidate by candidate.
  constexpr int CAND = DP > 32 ? KNN_CAND / 2 : KNN_CAND;
  bool quiet = false;
  pair_scan<DP>(a, q, tile, [&](int j0, int n) { ot_stage_h(a, th, j0, n); },
                [&](int j, int row, bool in, float c) {
                  if ((row & (CAND - 1)) == 0) quiet = otseg_quiet(w, j, CAND);   // the same for every lane, as are the boundaries
                  const float t = ot_t(c, a.s, th[row]);
                  if (quiet) otseg_add(w, t);
                  else if (in) {   // rows past the chunk's end: computed, never added
                    otseg_advance(w, j, a.seg_ptr, a.n_seg, out, live);
                    otseg_add(w, t);
                  }
                });
  otseg_finish(w, a.n_seg, out, live);
}

// grid (query tiles, n_seg), KNN_TQ threads: the chunks' states of one (segment, query) in chunk order into L
__global__ __launch_bounds__(KNN_TQ) void otseg_merge_kernel(const OtSegArgs a) {
  const long i = (long)blockIdx.x * KNN_TQ + threadIdx.x;
  const int s = blockIdx.y;
  if (i >= a.n_q) return;
  a.L[s * a.ld_l + i] = otseg_merge(a.ws + (long)s * a.n_q + i, (long)a.n_seg * a.n_q, a.n_split);
}

}  // namespace spv
