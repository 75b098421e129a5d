// Exact t-SNE of a low-dimensional layout (spv_tsne_repulsion, spv_tsne_affinities, spv_tsne_update; spVIPES.latent_tsne / spVIPES.tsne
// of the user API).  The expensive half of a t-SNE gradient is an all-pairs reduction over the layout's points -- the repulsive forces
// and the normaliser Z -- and that is pair_scan of spv_pair_scan.h with one more reduction: no tree, no grid, nothing of size n x n.
//
//   per pair   d2 = knn_d2 (spv_knn's chain, the same bits: the padding to DP = 4 adds fmaf(0, 0, acc) == acc)
//              w  = fl32(1 / fl32(1 + d2))        the correctly rounded quotient (tsne_w)
//              w2 = fl32(w * w)
//   Zrow[i]   += (double) w
//   F[t][i]   += (double) fl32(w2 * fl32(q_t - c_t))                                t < D
//
// How the work is laid out on the chip: pair_scan<4>, which states the layout (one query per lane, the grid (query tiles) x (chunks),
// the chunk through LDS 64 candidates at a time: 1 KiB).  Each lane keeps 1 + D fp64 running sums; the candidate's coordinates for the
// force are the 16 bytes of the LDS tile row pair_scan hands to `visit`, the same address for every lane (a broadcast read).
//   * n_split > 1: every (query tile, chunk) writes its 1 + D sums into the workspace [chunk][1 + D][n_q] and tsne_merge_kernel, one lane
//     per (query, sum), adds the chunks' values in chunk order from +0.  n_split == 1 writes Zrow / F directly: one launch.
// Order of addition: ascending candidate within a chunk, ascending chunk across chunks, no floating-point atomics.  For fixed shapes and
// n_split two calls agree bit for bit, and a query's sums do not depend on the other queries of the call.  Different n_split may differ
// in the last bits of fp64, except where every partial sum is exact.
//
// The perplexity calibration (tsne_affinities_kernel) and the sparse half with the step (tsne_zsum_kernel, tsne_update_kernel) are one
// lane per row, fp64, fixed order: their cost is a few per cent of the scan's.
//
// Registers and occupancy: the table at tsne_partial_kernel.
//
// The part between the two TSNE-CORE marks is plain C++ apart from __host__ __device__ and the rounding intrinsics:
// tools/tsne_host_check.py compiles exactly that text, after the KNN-CORE text it builds on, for the CPU.
#pragma once
#include "spv_knn.h"

namespace spv {

// ---- TSNE-CORE-BEGIN ----
constexpr int TSNE_DMAX = 4;          // SPV_TSNE_DMAX: the layout's dimensions, and the scan's DP
constexpr int TSNE_SEARCH_STEPS = 100;
constexpr double TSNE_SEARCH_TOL = 1e-5;

// the Student-t weight of a pair from its squared distance: two roundings
__host__ __device__ __forceinline__ float tsne_w(float d2) { return __fdiv_rn(1.f, __fadd_rn(1.f, d2)); }

// a lane's running sums over its chunk
struct TsneSums { double z; double f[TSNE_DMAX]; };
__host__ __device__ __forceinline__ void tsne_sums_init(TsneSums& s) {
  s.z = 0.0;
  for (int t = 0; t < TSNE_DMAX; ++t) s.f[t] = 0.0;
}

// one candidate joins: q, c are the padded vectors (zeros from D on: those sums stay +0 and are never written)
__host__ __device__ __forceinline__ void tsne_add(TsneSums& s, const float* q, const float* c, float d2) {
  const float w = tsne_w(d2), w2 = __fmul_rn(w, w);
  s.z += (double)w;
  for (int t = 0; t < TSNE_DMAX; ++t) s.f[t] += (double)__fmul_rn(w2, __fsub_rn(q[t], c[t]));
}

// the chunks' partial sums of one (sum, query), `st` apart, added in chunk order from +0
__host__ __device__ __forceinline__ double tsne_merge(const double* part, long st, int n_split) {
  double sum = 0.0;
  for (int c = 0; c < n_split; ++c) sum += part[c * st];
  return sum;
}

// chunks of the candidates = workgroups per query tile; a pure function of the shapes, knn_splits' plan with a target of its own: a
// chunk's state is 1 + D doubles, so chunks are cheap, and 16 workgroups fit a CU (8 waves per SIMD): two rounds of the 4096 resident.
constexpr int TSNE_TARGET_WG = 8192;
inline int tsne_splits(int n_q, int n_c) {
  if (n_q < 1 || n_c < 1) return 1;
  const long long tiles = ((long long)n_q + KNN_TQ - 1) / KNN_TQ;
  if (tiles >= TSNE_TARGET_WG) return 1;
  int s = (int)((TSNE_TARGET_WG + tiles - 1) / tiles);
  const int most = n_c / (KNN_MIN_TILES * KNN_TC);
  if (s > most) s = most;
  if (s > KNN_SPLIT_MAX) s = KNN_SPLIT_MAX;
  return s < 1 ? 1 : s;
}

// bytes of [n_split][1 + D][n_q] doubles; 0 for one chunk or a non-positive shape
inline long long tsne_ws_bytes(int n_q, int D, int n_split) {
  if (n_q < 1 || D < 1 || n_split <= 1) return 0;
  return (long long)n_split * (1 + D) * n_q * 8;
}

// ---- the perplexity calibration of one row: d2[0 .. k) ascending squared distances (+inf: an empty slot, which does not count)
// S = sum_j e_j, T = sum_j d_j e_j with e_j = exp(-beta d_j), d_j = d2[j] - d2[0], in ascending j; the entropy H = log S + beta T / S
__host__ __device__ __forceinline__ double tsne_entropy(const float* d2, int k, double beta, double& S) {
  const double d0 = (double)d2[0];
  double T = 0.0;
  S = 0.0;
  for (int j = 0; j < k; ++j) {
    if (!(d2[j] < INFINITY)) continue;
    const double d = (double)d2[j] - d0, e = exp(-beta * d);
    S += e;
    T += d * e;
  }
  return log(S) + beta * T / S;
}

// the binary search for beta: from 1, at most TSNE_SEARCH_STEPS steps, stop at |H - log(perplexity)| <= TSNE_SEARCH_TOL; beta doubles
// (halves) while its upper (lower) bound is infinite, else goes to the midpoint.  P[j] = fl32(e_j / S); an empty slot gets 0.
// A row without a finite slot gets beta = 1 and zeros.
__host__ __device__ __forceinline__ double tsne_calibrate(const float* d2, int k, double log_perp, float* P) {
  double beta = 1.0, lo = -INFINITY, hi = INFINITY, S = 0.0;
  if (k < 1 || !(d2[0] < INFINITY)) {
    for (int j = 0; j < k; ++j) P[j] = 0.f;
    return beta;
  }
  for (int l = 0; l < TSNE_SEARCH_STEPS; ++l) {
    const double diff = tsne_entropy(d2, k, beta, S) - log_perp;
    if (fabs(diff) <= TSNE_SEARCH_TOL) break;
    if (diff > 0.0) {
      lo = beta;
      beta = hi == INFINITY ? beta * 2.0 : (beta + hi) / 2.0;
    } else {
      hi = beta;
      beta = lo == -INFINITY ? beta / 2.0 : (beta + lo) / 2.0;
    }
  }
  tsne_entropy(d2, k, beta, S);   // the sum of the beta that is returned (after a last step it is a new one)
  const double d0 = (double)d2[0];
  for (int j = 0; j < k; ++j) P[j] = d2[j] < INFINITY ? (float)(exp(-beta * ((double)d2[j] - d0)) / S) : 0.f;
  return beta;
}

// ---- the sparse half of one row and its step
// the attractive term and the row's share of the KL divergence over the row's entries (cols ascending), in entry order from +0:
//   A[t] += (double) fl32(fl32(p w) fl32(y_i,t - y_j,t)),   kl += (double) p (log (double) p - log (double) w)      (p > 0)
// with w = tsne_w(knn_d2(y_i, y_j)).  A column outside [0, n) is skipped.
__host__ __device__ __forceinline__ void tsne_attract(const float* y, long ld_y, int n, int D, long i, const int* cols, const float* vals, long e0,
                                                      long e1, double* A, double& kl) {
  float yi[TSNE_DMAX], yj[TSNE_DMAX];
  for (int t = 0; t < TSNE_DMAX; ++t) { yi[t] = t < D ? y[i * ld_y + t] : 0.f; A[t] = 0.0; }
  kl = 0.0;
  for (long e = e0; e < e1; ++e) {
    const int j = cols[e];
    if (j < 0 || j >= n) continue;
    for (int t = 0; t < TSNE_DMAX; ++t) yj[t] = t < D ? y[(long)j * ld_y + t] : 0.f;
    const float p = vals[e], w = tsne_w(knn_d2(yi, yj, TSNE_DMAX)), pw = __fmul_rn(p, w);
    for (int t = 0; t < TSNE_DMAX; ++t) A[t] += (double)__fmul_rn(pw, __fsub_rn(yi[t], yj[t]));
    if (p > 0.f) kl += (double)p * (log((double)p) - log((double)w));
  }
}

// the gradient of one coordinate, fp64: g = 4 (alpha A - F / Z)
__host__ __device__ __forceinline__ double tsne_grad(double alpha, double A, double F, double Z) { return 4.0 * (alpha * A - F / Z); }

// the step of one coordinate: the gain grows by 0.2 where u g < 0 and shrinks to 0.8 of itself elsewhere, floor min_gain, stored in
// fp32; u = fl32(momentum u - lr gain g) with the stored gain; y = fl32(y + u) with the stored u
__host__ __device__ __forceinline__ float tsne_step(float y, float& u, float& gain, double g, double momentum, double lr, double min_gain) {
  double gn = (double)u * g < 0.0 ? (double)gain + 0.2 : (double)gain * 0.8;
  if (gn < min_gain) gn = min_gain;
  gain = (float)gn;
  u = (float)(momentum * (double)u - lr * (double)gain * g);
  return (float)((double)y + (double)u);
}

constexpr int TSNE_ZSUM_T = 256;   // lanes of the one workgroup that sums Zrow
// lane l's share of Zrow: elements l, l + TSNE_ZSUM_T, ... in ascending order from +0
__host__ __device__ __forceinline__ double tsne_zsum_lane(const double* Zrow, int n, int l) {
  double s = 0.0;
  for (long i = l; i < n; i += TSNE_ZSUM_T) s += Zrow[i];
  return s;
}
// the lanes' shares into one: a pairwise tree, part[l] += part[l + h] for h = T / 2, T / 4, .. 1
__host__ __device__ __forceinline__ void tsne_zsum_fold(double* part, int l, int h) { part[l] += part[l + h]; }
// ---- TSNE-CORE-END ----

struct TsneArgs {
  const float* Q; long ld_q; int n_q;
  const float* C; long ld_c; int n_c;
  int D;
  const int* exclude;
  int n_split, per;          // chunks, candidates per chunk
  double* Zrow;              // [n_q]
  double* F; long ld_f;      // [D][ld_f]
  double* ws;                // [n_split][1 + D][n_q] (n_split > 1)
};

// grid (query tiles, n_split), KNN_TQ threads, 1 KiB of static LDS.
//   VGPRs   SGPRs   scratch   waves per SIMD   workgroups per CU (2 waves each; the LDS would allow 64)
//     47      44       0           8                16
// (tsne_affinities_kernel: 68 VGPRs, 7 waves; tsne_update_kernel: 59, 8 waves; neither has scratch)
// (what the compiler reports for this text with the build's flags.  The quotient is v_rcp_f32 with the fma correction steps and
// v_div_fixup; the five sums are v_add_f64 behind v_cvt_f64_f32.)
__global__ __launch_bounds__(KNN_TQ) void tsne_partial_kernel(const TsneArgs a) {
  __shared__ __align__(16) float tile[KNN_TC * TSNE_DMAX];
  const int lane = threadIdx.x;
  const long i = (long)blockIdx.x * KNN_TQ + lane;
  const bool live = i < a.n_q;

  float q[TSNE_DMAX];
  scan_load_query<TSNE_DMAX>(a, i, live, q);
  const int ex = (live && a.exclude) ? a.exclude[i] : -1;
  TsneSums s;
  tsne_sums_init(s);

  pair_scan<TSNE_DMAX>(a, q, tile, [&](int j, int row, bool in, float d2) {   // rows past the chunk's end: computed, never added
    if (in && j != ex) {
      const f4v c = *reinterpret_cast<const f4v*>(tile + row * TSNE_DMAX);
      const float cv[TSNE_DMAX] = {c[0], c[1], c[2], c[3]};
      tsne_add(s, q, cv, d2);
    }
  });
  if (!live) return;
  if (a.n_split == 1) {
    a.Zrow[i] = s.z;
#pragma unroll
    for (int t = 0; t < TSNE_DMAX; ++t)
      if (t < a.D) a.F[t * a.ld_f + i] = s.f[t];
  } else {
    double* const out = a.ws + (long)blockIdx.y * (1 + a.D) * a.n_q + i;
    out[0] = s.z;
#pragma unroll
    for (int t = 0; t < TSNE_DMAX; ++t)
      if (t < a.D) out[(long)(1 + t) * a.n_q] = s.f[t];
  }
}

// grid (query tiles, 1 + D), KNN_TQ threads: the chunks' values of one (sum, query) in chunk order into Zrow / F
__global__ __launch_bounds__(KNN_TQ) void tsne_merge_kernel(const TsneArgs a) {
  const long i = (long)blockIdx.x * KNN_TQ + threadIdx.x;
  const int r = blockIdx.y;
  if (i >= a.n_q) return;
  const double v = tsne_merge(a.ws + (long)r * a.n_q + i, (long)(1 + a.D) * a.n_q, a.n_split);
  if (r == 0) a.Zrow[i] = v;
  else a.F[(r - 1) * a.ld_f + i] = v;
}

struct TsneAffArgs { const float* d2; float* P; long ld; int n, k; double log_perp; double* beta; };

// grid (rows / 128), 128 threads: one lane per row
__global__ __launch_bounds__(128) void tsne_affinities_kernel(const TsneAffArgs a) {
  const long i = (long)blockIdx.x * 128 + threadIdx.x;
  if (i >= a.n) return;
  a.beta[i] = tsne_calibrate(a.d2 + i * a.ld, a.k, a.log_perp, a.P + i * a.ld);
}

struct TsneUpdArgs {
  const float* y_in; float* y_out; long ld_y; int n, D;
  const long* indptr; const int* cols; const float* vals;
  const double* Zrow; const double* F; long ld_f;
  double* Z;
  float* u; float* gain;
  double alpha, momentum, lr, min_gain;
  double* kl_row; double* grad;
};

// one workgroup of TSNE_ZSUM_T threads: Z[0] = the sum of Zrow in a fixed order
__global__ __launch_bounds__(TSNE_ZSUM_T) void tsne_zsum_kernel(const TsneUpdArgs a) {
  __shared__ double part[TSNE_ZSUM_T];
  const int l = threadIdx.x;
  part[l] = tsne_zsum_lane(a.Zrow, a.n, l);
  for (int h = TSNE_ZSUM_T / 2; h >= 1; h /= 2) {
    __syncthreads();
    if (l < h) tsne_zsum_fold(part, l, h);
  }
  if (l == 0) a.Z[0] = part[0];
}

// grid (rows / 128), 128 threads: one lane per row of P
__global__ __launch_bounds__(128) void tsne_update_kernel(const TsneUpdArgs a) {
  const long i = (long)blockIdx.x * 128 + threadIdx.x;
  if (i >= a.n) return;
  double A[TSNE_DMAX], kl;
  tsne_attract(a.y_in, a.ld_y, a.n, a.D, i, a.cols, a.vals, a.indptr[i], a.indptr[i + 1], A, kl);
  const double Z = a.Z[0];
#pragma unroll
  for (int t = 0; t < TSNE_DMAX; ++t) {
    if (t >= a.D) break;
    const double g = tsne_grad(a.alpha, A[t], a.F[t * a.ld_f + i], Z);
    float u = a.u[i * a.ld_y + t], gain = a.gain[i * a.ld_y + t];
    a.y_out[i * a.ld_y + t] = tsne_step(a.y_in[i * a.ld_y + t], u, gain, g, a.momentum, a.lr, a.min_gain);
    a.u[i * a.ld_y + t] = u;
    a.gain[i * a.ld_y + t] = gain;
    if (a.grad) a.grad[(long)t * a.n + i] = g;
  }
  if (a.kl_row) a.kl_row[i] = kl;
}

}  // namespace spv
