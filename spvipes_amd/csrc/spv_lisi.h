// LISI, the local inverse Simpson index of Korsunsky et al. (spv_lisi; spVIPES.latent_lisi / spVIPES.lisi of the user API): for every
// cell the effective number of labels among its nearest neighbours, from the neighbour lists spv_knn_paged writes.  One kernel calibrates
// the Gaussian kernel width of a cell to the perplexity and computes the Simpson index of up to LISI_SETS_MAX label sets on that one
// calibration (iLISI over the groups and cLISI over the labels share it).
//
//   per slot j of the row   r_j = (double) fl32(sqrt(dist_j))  (the correctly rounded fp32 root: the distance latent_neighbors reports),
//                           d_j = r_j - r_0; a slot whose dist is not < +inf does not count (e_j = p_j = 0)
//   per beta                S = sum_j e_j, T = sum_j d_j e_j, e_j = exp(-beta d_j), H = log S + beta T / S
//   the search              beta = 1; up to LISI_STEPS updates while |H - log(perplexity)| >= LISI_TOL: beta doubles (halves) while its
//                           upper (lower) bound is infinite, else goes to the midpoint (compute_simpson of the published code)
//   p_j = e_j / S,          simpson = sum_j p_j s_j with s_j = sum_j' p_j' [code_j' == code_j] over the slots whose code is >= 0
//   lisi = 1 / simpson
// d_0 = 0, so S >= 1 for every beta: the underflow case of the published code (S == 0) does not exist.  A row whose slot 0 is not finite
// (the lists are ascending: an empty row) gets lisi = NaN, beta = 1, n_valid = 0, converged = 0.
//
// How the work is laid out on the chip
//   * One wave per row, LISI_WAVES = 4 rows per workgroup.  Lane l holds the slots l, l + 64, l + 128, l + 192 (below k): coalesced reads
//     of idx / dist, and d_j stays in LISI_SLOTS = 4 registers through the whole search.
//   * EVERY sum over the slots -- S, T, simpson, n_valid -- has ONE order: the lane adds its slots in ascending slot from +0, then the 64
//     lane values fold by a butterfly, x += shfl_xor(x, m) for m = 32, 16, 8, 4, 2, 1.  Addition commutes, so after every round both
//     partners hold the same bits, and after the last every lane holds the same value: the search's branches are wave-uniform, and nothing
//     of it passes through memory.  No atomics; a row's values do not depend on the other rows of the call.
//   * The per-label sums need no table of labels and put no limit on their number: p_j (once) and code_j (per label set) go to LDS, and the
//     lane of slot j adds s_j = sum_j' p_j' [code_j' == code_j] over j' = 0 .. k-1 in ascending j' from +0 (every lane reads the same
//     address: a broadcast).  A slot that does not match adds +0, which leaves the bits of a sum that is never -0.  Only equality of codes
//     is ever asked, so renaming the codes leaves every bit unchanged.
//   * LDS: 4 x 256 x (8 + 4) bytes = 12 KiB per workgroup.  The two barriers per label set are taken by all four waves the same number of
//     times (n_sets is uniform); the search, whose trip count differs per row, touches no LDS.
// Registers and occupancy: the table at lisi_kernel.
//
// The part between the two LISI-CORE marks is plain C++ apart from __host__ __device__:
// tools/lisi_host_check.py compiles exactly that text for the CPU and plays the 64 lanes and the butterfly in the same order.
#pragma once
#include "spv_common.h"
#include <cmath>

namespace spv {

// ---- LISI-CORE-BEGIN ----
constexpr int LISI_KMAX = 256;      // SPV_LISI_KMAX (= SPV_KNN_PAGED_KMAX)
constexpr int LISI_SETS_MAX = 8;    // SPV_LISI_SETS_MAX
constexpr int LISI_LANES = 64;
constexpr int LISI_SLOTS = LISI_KMAX / LISI_LANES;   // slots per lane
constexpr int LISI_WAVES = 4;       // rows per workgroup
constexpr int LISI_STEPS = 50;      // updates of beta at most
constexpr double LISI_TOL = 1e-5;

// the distance of a slot from its squared fp32 distance: sqrtf, which the build's flags compile to the correctly rounded root (as
// sil_root of spv_silhouette.h; the bare 1-ulp instruction is what the _rn intrinsic gives)
__host__ __device__ __forceinline__ double lisi_root(float d2) { return (double)sqrtf(d2); }

// a lane's share of S and T: its slots in ascending slot from +0; d[m] < 0 marks a slot that does not count (every real d is >= 0)
__host__ __device__ __forceinline__ void lisi_lane_sums(const double* d, double beta, double& S, double& T) {
  S = 0.0;
  T = 0.0;
  for (int m = 0; m < LISI_SLOTS; ++m) {
    if (!(d[m] >= 0.0)) continue;
    const double e = exp(-beta * d[m]);
    S += e;
    T += d[m] * e;
  }
}

__host__ __device__ __forceinline__ double lisi_entropy(double S, double T, double beta) { return log(S) + beta * T / S; }

// one update of the search, diff = H - log(perplexity)
__host__ __device__ __forceinline__ void lisi_update(double diff, double& beta, double& lo, double& hi) {
  if (diff > 0.0) {
    lo = beta;
    beta = hi == INFINITY ? beta * 2.0 : (beta + hi) / 2.0;
  } else {
    hi = beta;
    beta = lo == -INFINITY ? beta / 2.0 : (beta + lo) / 2.0;
  }
}

// the affinity of a slot at the final beta (0 for a slot that does not count)
__host__ __device__ __forceinline__ double lisi_p(double d, double beta, double S) { return d >= 0.0 ? exp(-beta * d) / S : 0.0; }

// s_j of a slot with code c >= 0: the affinities of the k slots with the same code, ascending from +0
__host__ __device__ __forceinline__ double lisi_same(const double* p, const int* code, int k, int c) {
  double s = 0.0;
  for (int j = 0; j < k; ++j) s += code[j] == c ? p[j] : 0.0;
  return s;
}

// a lane's share of the Simpson index: p_j s_j over its slots l, l + 64, .. < k in ascending slot from +0; a negative code adds nothing
__host__ __device__ __forceinline__ double lisi_lane_simpson(const double* p, const int* code, int k, int l) {
  double v = 0.0;
  for (int m = 0; m < LISI_SLOTS; ++m) {
    const int j = l + m * LISI_LANES;
    if (j < k && code[j] >= 0) v += p[j] * lisi_same(p, code, k, code[j]);
  }
  return v;
}
// ---- LISI-CORE-END ----

struct LisiArgs {
  const int* idx; const float* dist; long ld; int n, k;
  const int* codes; int n_c, n_sets;     // [n_sets][n_c]
  double log_perp;
  double* lisi;                          // [n_sets][n]
  double* beta; int* n_valid; int* converged;   // [n]
};

__device__ __forceinline__ double lisi_fold(double x) {
#pragma unroll
  for (int m = LISI_LANES / 2; m >= 1; m /= 2) x += __shfl_xor(x, m, LISI_LANES);
  return x;
}
__device__ __forceinline__ int lisi_fold(int x) {
#pragma unroll
  for (int m = LISI_LANES / 2; m >= 1; m /= 2) x += __shfl_xor(x, m, LISI_LANES);
  return x;
}

// grid (rows / LISI_WAVES), LISI_WAVES * 64 threads, 12 KiB of static LDS
//   VGPRs   SGPRs   scratch   waves per SIMD   LDS per workgroup
//     83      82       0           5                12288
// (what the compiler reports for this text with the build's flags)
__global__ __launch_bounds__(LISI_WAVES * LISI_LANES) void lisi_kernel(const LisiArgs a) {
  __shared__ double p_s[LISI_WAVES][LISI_KMAX];
  __shared__ int c_s[LISI_WAVES][LISI_KMAX];
  const int w = threadIdx.x / LISI_LANES, l = threadIdx.x % LISI_LANES, k = a.k;
  const long i = (long)blockIdx.x * LISI_WAVES + w;
  const bool live = i < a.n;   // wave-uniform

  double d[LISI_SLOTS];
  int nb[LISI_SLOTS] = {-1, -1, -1, -1};
  double beta = 1.0, S = 1.0;
  bool any = false;
  if (live) {
    const float first = a.dist[i * a.ld];
    any = first < INFINITY;
    const double r0 = lisi_root(first);
    int cnt = 0;
#pragma unroll
    for (int m = 0; m < LISI_SLOTS; ++m) {
      const int j = l + m * LISI_LANES;
      const float d2 = j < k ? a.dist[i * a.ld + j] : INFINITY;
      const bool ok = any && d2 < INFINITY;
      nb[m] = (ok && j < k) ? a.idx[i * a.ld + j] : -1;
      d[m] = ok ? lisi_root(d2) - r0 : -1.0;
      if (ok && !(d[m] >= 0.0)) d[m] = 0.0;   // a list that does not ascend: no slot is nearer than slot 0
      cnt += ok;
    }
    cnt = lisi_fold(cnt);
    int conv = 0;
    if (any) {
      double lo = -INFINITY, hi = INFINITY, T, diff;
      for (int tries = 0;; ++tries) {
        lisi_lane_sums(d, beta, S, T);
        S = lisi_fold(S);
        T = lisi_fold(T);
        diff = lisi_entropy(S, T, beta) - a.log_perp;
        if (fabs(diff) < LISI_TOL || tries == LISI_STEPS) break;
        lisi_update(diff, beta, lo, hi);
      }
      conv = fabs(diff) < LISI_TOL;
    }
    if (l == 0) { a.beta[i] = beta; a.n_valid[i] = cnt; a.converged[i] = conv; }
#pragma unroll
    for (int m = 0; m < LISI_SLOTS; ++m) p_s[w][l + m * LISI_LANES] = any ? lisi_p(d[m], beta, S) : 0.0;
  }
  for (int t = 0; t < a.n_sets; ++t) {
    if (live) {
#pragma unroll
      for (int m = 0; m < LISI_SLOTS; ++m)
        c_s[w][l + m * LISI_LANES] = (nb[m] >= 0 && nb[m] < a.n_c) ? a.codes[(long)t * a.n_c + nb[m]] : -1;
    }
    __syncthreads();
    if (live) {
      const double simpson = lisi_fold(lisi_lane_simpson(p_s[w], c_s[w], k, l));
      if (l == 0) a.lisi[(long)t * a.n + i] = any ? 1.0 / simpson : NAN;
    }
    __syncthreads();
  }
}

}  // namespace spv
