// Expected-expression statistics: decode and REDUCE over the cells of a population in one entry point (spv_dec_expected_stats;
// expression_statistics of the user API).
//
// The values are spv_dec_expected's for what = 0, 1, 2, 3 at alpha = 1, bit for bit: dec_expected_kernel's front end (dx_stage_am,
// load_ps_cell_frags, dx_tile_gene, dx_decode_tile) and dx_value itself.  Nothing of size cells x genes is stored:
//   * the caller hands in cells that are already arranged by segment: tile t (32 consecutive operand rows, one workgroup) belongs to
//     segment tile_seg[t] and its first tile_n[t] rows count.  A tile whose code is negative or >= n_seg, whose count is <= 0 or
//     whose rows all lie at or beyond B is skipped by the whole workgroup ahead of its staging barrier.
//   * per gene tile a wave turns the four values, one after the other, through its ONE LDS transpose tile (the tile of the store
//     stage of dec_expected_kernel: the LDS footprint and with it the occupancy stay that kernel's).  With lane = gene r, half h sums
//     the counted cells h, h + 2, ... in ascending order in fp64 -- every fp32 value is widened first, its square is formed in fp64
//     and is exact -- then the two halves are added as (even cells) + (odd cells).  The eight sums of the gene go to
//     ws[cell tile][8][n_genes] with 256-byte coalesced stores: rows 0..3 = sum of mixture mean, private part, shared part, mixing
//     weight, rows 4..7 = the sums of their squares.
//   * dec_expected_stats_merge_kernel then walks the cell tiles in ascending order, one thread per (row, gene), and adds every run of
//     tiles of one segment onto stats[segment][row][gene].  Each table element has one writer.
// There are no floating-point atomics and every order of addition is fixed by the tile arrays: two calls agree bit for bit.
// The loops keep spv_dec_expected.h's rules: fixed trip counts, no barrier in divergent code, the wave-local hand-over through
// dx_wave_sync.
#pragma once
#include "spv_dec_expected.h"

namespace spv {

constexpr int DXS_ROWS = 8;   // sums per (segment, gene): four values, four squares

struct DecExpStatsArgs {
  const bf16_t *Am_hi, *Am_lo, *Wm_hi, *Wm_lo;   // [Bp][K], [Gp][K]
  int K;
  const int* genes; int n_genes; int n_seg;
  const int* tile_seg; const int* tile_n;        // one entry per 32-cell tile with a row below B
  double* ws;                                    // [Bp / 32][8][n_genes]
};

// how many rows of cell tile t are counted: 0 = the tile is skipped (the arrays are not read for a tile wholly at or beyond row B)
__device__ __forceinline__ int dxs_tile_count(const int* tile_seg, const int* tile_n, int t, int n_seg, int B) {
  const int left = B - t * DX_CELLS;
  if (left <= 0) return 0;
  const int sg = tile_seg[t];
  if (sg < 0 || sg >= n_seg) return 0;
  return max(min(min(tile_n[t], DX_CELLS), left), 0);
}

template <int NSPLIT, int KW>
__global__ __launch_bounds__(256) void dec_expected_stats_kernel(DecParams p, DecExpStatsArgs a) {
  __shared__ __attribute__((aligned(16))) bf16_t s_am[(NSPLIT == 3 ? 2 : 1) * DX_PLANE];
  __shared__ __attribute__((aligned(16))) float s_t[4][32 * DX_TPITCH];
  const int nct = dxs_tile_count(a.tile_seg, a.tile_n, blockIdx.x, a.n_seg, p.B);
  if (nct == 0) return;   // (the whole workgroup, ahead of the barrier)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, r = lane & 31;
  const int cell0 = blockIdx.x * DX_CELLS;   // (cell0 + 32 <= Bp: the grid has Bp / 32 columns)
  dx_stage_am<NSPLIT>(s_am, a.Am_hi, a.Am_lo, a.K, cell0, tid);
  PsFragsK<KW> cf;
  load_ps_cell_frags(p, cell0, lane, cf);
  const float ap = p.a_p[cell0 + r], as = p.a_s[cell0 + r];
  __syncthreads();
  const int ntiles = (a.n_genes + 31) >> 5;
  float* const tile = s_t[wave];
  const bf16_t* const arow = s_am + r * DX_APITCH + 8 * h;
  double* const part = a.ws + (long)blockIdx.x * DXS_ROWS * a.n_genes;
  for (int t = blockIdx.y * 4 + wave; t < ntiles; t += gridDim.y * 4) {
    const int sel0 = t * 32, col = sel0 + r;
    f16v yp, ys, acc;
    dx_decode_tile<NSPLIT, KW>(p.Wps_hi, p.Wps_lo, a.Wm_hi, a.Wm_lo, a.K, dx_tile_gene(a.genes, a.n_genes, sel0, r, p.G), h, arow, cf, yp, ys, acc);
#pragma unroll
    for (int q = 0; q < 16; ++q) { yp[q] = __expf(yp[q] + ap); ys[q] = __expf(ys[q] + as); }   // the two rates, as dec_expected_kernel forms them
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      // ---- value w -> the wave's LDS tile [cell r][gene crow(q, h)] -------------------------------------------------------
#pragma unroll
      for (int qq = 0; qq < 4; ++qq) {
        f4v v;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int q = 4 * qq + j;
          v[j] = dx_value(w, yp[q], ys[q], acc[q]);
        }
        *reinterpret_cast<f4v*>(tile + r * DX_TPITCH + 8 * qq + 4 * h) = v;
      }
      dx_wave_sync();
      // ---- sum with lane = gene: counted rows 2 i + h in ascending order, then (even rows) + (odd rows) ------------------------
      double s = 0.0, sq = 0.0;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int c = 2 * i + h;
        const double x = (double)tile[c * DX_TPITCH + r];
        if (c < nct) { s += x; sq += x * x; }
      }
      const double os = __shfl_xor(s, 32), osq = __shfl_xor(sq, 32);
      const double ts = h ? os + s : s + os, tq = h ? osq + sq : sq + osq;
      if (col < a.n_genes) part[(long)(h ? 4 + w : w) * a.n_genes + col] = h ? tq : ts;   // half 0: the sum's row, half 1: the squares' row
      dx_wave_sync();   // the tile is rewritten by the next value / the next iteration
    }
  }
}

// stats[segment][row][gene] += the segment's tile partials, in ascending tile order; one thread per (row, gene)
__global__ __launch_bounds__(256) void dec_expected_stats_merge_kernel(const int* tile_seg, const int* tile_n, int n_cell_tiles, int n_seg, int B,
                                                                       int n_genes, const double* ws, double* stats, long ld_stats) {
  const int j = blockIdx.x * 256 + threadIdx.x, row = blockIdx.y;
  if (j >= n_genes) return;
  int cur = -1;
  double run = 0.0;
  for (int t = 0; t < n_cell_tiles; ++t) {
    if (dxs_tile_count(tile_seg, tile_n, t, n_seg, B) == 0) continue;   // (uniform: every thread walks the same tiles)
    const int sg = tile_seg[t];
    if (sg != cur) {
      if (cur >= 0) stats[((long)cur * DXS_ROWS + row) * ld_stats + j] += run;
      cur = sg; run = 0.0;
    }
    run += ws[((long)t * DXS_ROWS + row) * n_genes + j];
  }
  if (cur >= 0) stats[((long)cur * DXS_ROWS + row) * ld_stats + j] += run;
}

}  // namespace spv
