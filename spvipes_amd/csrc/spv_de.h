// Differential expression, "change" mode: per gene the statistics of lfc_m = log2(x1 + eps) - log2(x2 + eps) over n_pairs pairs of
// rows drawn from two device-resident sample banks (spv_de_pairs; spVIPES.differential_expression of the user API).
//
// How the work is laid out on the chip
//   * Lanes run along genes: a wave owns 64 consecutive genes and a contiguous chunk of pairs.  A pair's two row numbers are
//     wave-uniform (read through the scalar path, clamped there), so one pair costs the wave two 256-byte row pieces and no address
//     arithmetic per lane.  DE_UNROLL pairs = 2 * DE_UNROLL independent loads are issued before the first is used: the gathers are
//     the whole cost.
//   * A workgroup = 4 waves on one gene tile and one "split" of the pairs; the grid is (gene tiles) x (splits), with the splits
//     chosen so that about DE_TARGET_WAVES waves exist whatever n_genes is (de_splits).  Workgroups of one gene tile are numbered
//     so that they land on one XCD (consecutive workgroup ids go round the 8 XCDs): the 4096 x 256 byte column block they all gather
//     from then sits in one L2.
//   * Reduction, in a fixed order throughout (no floating-point atomics; two calls agree bit for bit):
//       lane, fp32 : K = the chunk's first lfc, s = sum(lfc - K), q = sum((lfc - K)^2), min, max, count, sum x1, sum x2
//       wave       : (n, S = n K + s, M2 = q - s^2 / n) in fp64
//       workgroup  : waves 0..3 merged in that order with Chan's pairwise formula in fp64 -> one record per (split, gene) in `ws`
//       de_finish  : wave w of a 512-thread workgroup folds the records of splits w, w + 8, ... in order, waves 0..7 merged in order
//     The shift by K keeps a column with lfc = 20 +- 1e-2 at full fp32 resolution: the squares summed are those of ~1e-2, not of 20.
//     A constant column gives s = q = 0 exactly, hence std == 0 and mean == min == max.
#pragma once
#include "spv_common.h"
#include <cfloat>

namespace spv {

constexpr int DE_WAVES = 4;             // waves per workgroup of de_pairs_kernel
constexpr int DE_UNROLL = 8;            // pairs in flight per wave
constexpr int DE_FIN_WAVES = 8;         // waves per workgroup of de_finish_kernel
constexpr int DE_TARGET_WAVES = 6144;   // 24 per CU
constexpr int DE_MIN_PAIRS = 16;        // a wave is not worth fewer pairs than two unrolled rounds
constexpr int DE_FIELDS = 7;            // doubles per (split, gene) record: S, M2, min, max, count, sum x1, sum x2

struct DeArgs {
  const float *bank1, *bank2; long ld1, ld2;
  const int *rows1, *rows2; int n_rows1, n_rows2;
  int n_genes, n_pairs; float delta, eps;
  float* stats; long ld_stats;
  double* ws; int splits;
};

// splits of the pairs = workgroups per gene tile.  A lane's longest fp32 chain is ceil(ceil(n_pairs / splits) / 4) pairs.
inline int de_splits(int n_genes, int n_pairs) {
  const int tiles = (n_genes + 63) / 64;
  int waves = (DE_TARGET_WAVES + tiles - 1) / tiles;
  const int most = n_pairs / DE_MIN_PAIRS > 1 ? n_pairs / DE_MIN_PAIRS : 1;
  if (waves > most) waves = most;
  return (waves + DE_WAVES - 1) / DE_WAVES;   // (>= 1, and <= n_pairs: every workgroup has a pair)
}

struct DeAcc { double n, S, M2, mn, mx, cnt, s1, s2; };

// a <- a (+) b in that order (Chan, Golub, LeVeque: M2 of the union from the parts' sizes, sums and M2); n is wave-uniform
__device__ __forceinline__ void de_merge(DeAcc& a, const DeAcc& b) {
  if (b.n == 0.0) return;
  if (a.n == 0.0) { a = b; return; }
  const double N = a.n + b.n, d = b.S / b.n - a.S / a.n;
  a.M2 += b.M2 + d * d * (a.n * b.n / N);
  a.S += b.S; a.n = N;
  a.mn = fmin(a.mn, b.mn); a.mx = fmax(a.mx, b.mx);
  a.cnt += b.cnt; a.s1 += b.s1; a.s2 += b.s2;
}

// waves 1 .. NW-1 hand their accumulators to wave 0, which merges them in wave order (all waves call; wave 0 holds the result)
template <int NW>
__device__ __forceinline__ void de_block_merge(DeAcc& a, double (*sm)[8][64], int wave, int lane) {
  if (wave > 0) {
    double* const o = &sm[wave][0][lane];
    o[0 * 64] = a.n; o[1 * 64] = a.S; o[2 * 64] = a.M2; o[3 * 64] = a.mn; o[4 * 64] = a.mx; o[5 * 64] = a.cnt; o[6 * 64] = a.s1; o[7 * 64] = a.s2;
  }
  __syncthreads();
  if (wave == 0) {
    for (int w = 1; w < NW; ++w) {
      const double* const i = &sm[w][0][lane];
      const DeAcc b{i[0 * 64], i[1 * 64], i[2 * 64], i[3 * 64], i[4 * 64], i[5 * 64], i[6 * 64], i[7 * 64]};
      de_merge(a, b);
    }
  }
}

struct DeLane { float K, s, q, mn, mx, s1, s2; int cnt; };

__device__ __forceinline__ float de_lfc(float x1, float x2, float eps) {
  // v_log_f32 (1 ulp); its operands are normal numbers by the max with FLT_MIN, so no denormal rescue is needed around it
  return __builtin_amdgcn_logf(fmaxf(x1 + eps, FLT_MIN)) - __builtin_amdgcn_logf(fmaxf(x2 + eps, FLT_MIN));
}

__device__ __forceinline__ void de_term(DeLane& l, float x1, float x2, float eps, float delta) {
  const float d = de_lfc(x1, x2, eps), t = d - l.K;
  l.s += t; l.q = fmaf(t, t, l.q);
  l.mn = fminf(l.mn, d); l.mx = fmaxf(l.mx, d);
  l.cnt += fabsf(d) >= delta ? 1 : 0;
  l.s1 += x1; l.s2 += x2;
}

__device__ __forceinline__ long de_row(const int* rows, int m, int n_rows, long ld) {
  const int r = min(max(rows[m], 0), n_rows - 1);   // (m is wave-uniform: a scalar load and scalar clamps)
  return (long)r * ld;
}

__global__ __launch_bounds__(256) void de_pairs_kernel(DeArgs a) {
  __shared__ double sm[DE_WAVES][8][64];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int tiles = (a.n_genes + 63) >> 6, nwg = tiles * a.splits;
  // workgroup ids id, id + 8, id + 16, ... share an XCD: give them consecutive work items (the grid is a multiple of 8)
  const int per = gridDim.x >> 3, w = (blockIdx.x & 7) * per + (blockIdx.x >> 3);
  if (w >= nwg) return;
  const int tile = w / a.splits, split = w - tile * a.splits;
  const int col = tile * 64 + lane, j = min(col, a.n_genes - 1);   // a lane beyond the last gene re-reads it and stores nothing
  // this wave's pairs: the split's share [p0, p1) cut in four
  const int p0 = (int)((long)split * a.n_pairs / a.splits), p1 = (int)((long)(split + 1) * a.n_pairs / a.splits);
  const int m0 = p0 + (int)((long)wave * (p1 - p0) / DE_WAVES), m1 = p0 + (int)((long)(wave + 1) * (p1 - p0) / DE_WAVES);
  const float* const b1 = a.bank1 + j;
  const float* const b2 = a.bank2 + j;
  DeAcc acc{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (m1 > m0) {
    DeLane l;
    {
      const float x1 = b1[de_row(a.rows1, m0, a.n_rows1, a.ld1)], x2 = b2[de_row(a.rows2, m0, a.n_rows2, a.ld2)];
      const float d = de_lfc(x1, x2, a.eps);
      l = DeLane{d, 0.f, 0.f, d, d, x1, x2, fabsf(d) >= a.delta ? 1 : 0};
    }
    int m = m0 + 1;
    for (; m + DE_UNROLL <= m1; m += DE_UNROLL) {
      float x1[DE_UNROLL], x2[DE_UNROLL];
#pragma unroll
      for (int u = 0; u < DE_UNROLL; ++u) {
        x1[u] = b1[de_row(a.rows1, m + u, a.n_rows1, a.ld1)];
        x2[u] = b2[de_row(a.rows2, m + u, a.n_rows2, a.ld2)];
      }
#pragma unroll
      for (int u = 0; u < DE_UNROLL; ++u) de_term(l, x1[u], x2[u], a.eps, a.delta);
    }
    for (; m < m1; ++m) de_term(l, b1[de_row(a.rows1, m, a.n_rows1, a.ld1)], b2[de_row(a.rows2, m, a.n_rows2, a.ld2)], a.eps, a.delta);
    const double n = (double)(m1 - m0), s = (double)l.s;
    acc = DeAcc{n, n * (double)l.K + s, fmax((double)l.q - s * s / n, 0.0), (double)l.mn, (double)l.mx, (double)l.cnt, (double)l.s1, (double)l.s2};
  }
  de_block_merge<DE_WAVES>(acc, sm, wave, lane);
  if (wave == 0 && col < a.n_genes) {   // (p1 > p0 for every split, so wave 0's merged record is never empty)
    double* const o = a.ws + (long)split * DE_FIELDS * a.n_genes + col;
    const long g = a.n_genes;
    o[0] = acc.S; o[g] = acc.M2; o[2 * g] = acc.mn; o[3 * g] = acc.mx; o[4 * g] = acc.cnt; o[5 * g] = acc.s1; o[6 * g] = acc.s2;
  }
}

__global__ __launch_bounds__(64 * DE_FIN_WAVES) void de_finish_kernel(DeArgs a) {
  __shared__ double sm[DE_FIN_WAVES][8][64];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int col = blockIdx.x * 64 + lane, j = min(col, a.n_genes - 1);
  const long g = a.n_genes;
  DeAcc acc{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int split = wave; split < a.splits; split += DE_FIN_WAVES) {
    const int p0 = (int)((long)split * a.n_pairs / a.splits), p1 = (int)((long)(split + 1) * a.n_pairs / a.splits);
    const double* const i = a.ws + (long)split * DE_FIELDS * g + j;
    const DeAcc b{(double)(p1 - p0), i[0], i[g], i[2 * g], i[3 * g], i[4 * g], i[5 * g], i[6 * g]};
    de_merge(acc, b);
  }
  de_block_merge<DE_FIN_WAVES>(acc, sm, wave, lane);
  if (wave == 0 && col < a.n_genes) {
    float* const o = a.stats + col;
    const long ld = a.ld_stats;
    o[0] = (float)(acc.S / acc.n); o[ld] = (float)sqrt(acc.M2 / acc.n);
    o[2 * ld] = (float)acc.mn; o[3 * ld] = (float)acc.mx; o[4 * ld] = (float)acc.cnt;
    o[5 * ld] = (float)(acc.s1 / acc.n); o[6 * ld] = (float)(acc.s2 / acc.n);
  }
}

}  // namespace spv
