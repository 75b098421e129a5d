// Posterior-predictive check: decode, draw and REDUCE in one kernel (spv_dec_sample_stats; posterior_predictive_check of the user API).
//
// The draws are spv_dec_sample's, integer for integer: dec_sample_kernel's front end (dx_stage_am, load_ps_cell_frags, dx_tile_gene,
// dx_decode_tile), its s_gid / s_th rows and its rolled draw loop with the same NbStream addressing (spv_dec_sample.h).  Every draw
// still lands in the wave's LDS tile [cell][gene]; from there on nothing of size cells x genes is stored:
//   * gene side -- the tile is read in the store stage's transposed order (lane = gene r, half h takes cells h, h + 2, ...).  Per gene
//     four values accumulate in registers over the tile's cells: sum, non-zero tally, sum of squares (modulo 2^64) and max.  A cell's
//     segment code comes from a 32-entry LDS row staged once per workgroup; the values are flushed to stats[seg][4][ld_stats] with
//     64-bit unsigned atomicAdd / atomicMax (results unused) when the code changes and at the end of the tile.  The two halves of a
//     gene are combined first when they end in the same segment; a flush whose sum is 0 is skipped (nothing to add, max 0).
//   * cell side -- in the draw loop (lane = cell) each lane adds its draws into a running total across all its tiles and issues one
//     64-bit atomicAdd into cell_total after the tile loop.
// Integer sums do not depend on the order of addition: the tables equal the reduction of spv_dec_sample's output bit for bit, and two
// calls agree bit for bit.  Cells with a negative code, a code >= n_seg, or a row >= B are neither drawn nor counted.
// The loops keep spv_dec_sample.h's rules: fixed trip caps, no barrier and no cross-lane operation inside the divergent draw loop
// (the one cross-lane exchange, the halves' combine, runs after the wave has reconverged).
#pragma once
#include "spv_dec_sample.h"

namespace spv {

typedef unsigned long long u64_t;

struct DecSampleStatsArgs {
  const bf16_t *Am_hi, *Am_lo, *Wm_hi, *Wm_lo;
  int K;
  const int* genes; int n_genes;
  const float* theta;       // [G] exp(px_r)
  const int* cell_ids;      // [B] or null
  unsigned long long key; unsigned sample;
  const int* seg; int n_seg;              // [B] or null (everything in segment 0)
  u64_t* stats; long ld_stats;            // [n_seg][4][ld_stats]: sum, non-zero tally, sum of squares mod 2^64, max
  u64_t* cell_total;                      // [B] or null
};

// one gene's partial of one segment -> the table (sg < 0: nothing pending; s == 0: every count was 0, nothing changes)
__device__ __forceinline__ void dss_flush(u64_t* stats, long ld, int sg, int col, u64_t s, unsigned nz, u64_t q, unsigned mx) {
  if (sg < 0 || s == 0) return;
  u64_t* const o = stats + (long)sg * 4 * ld + col;
  atomicAdd(o, s);
  atomicAdd(o + ld, (u64_t)nz);
  atomicAdd(o + 2 * ld, q);
  atomicMax(o + 3 * ld, (u64_t)mx);
}

template <int NSPLIT, int KW>
__global__ __launch_bounds__(256) void dec_sample_stats_kernel(DecParams p, DecSampleStatsArgs a) {
  __shared__ __attribute__((aligned(16))) bf16_t s_am[(NSPLIT == 3 ? 2 : 1) * DX_PLANE];
  __shared__ __attribute__((aligned(16))) int s_t[4][32 * DX_TPITCH];
  __shared__ int s_gid[4][32];
  __shared__ float s_th[4][32];
  __shared__ int s_seg[32];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, r = lane & 31;
  const int cell0 = blockIdx.x * DX_CELLS;   // (cell0 + 32 <= Bp: the grid has Bp / 32 columns)
  const bf16_t* const wps_hi = nbs_in_vgpr(p.Wps_hi), * const wps_lo = nbs_in_vgpr(p.Wps_lo);
  dx_stage_am<NSPLIT>(s_am, a.Am_hi, a.Am_lo, a.K, cell0, tid);
  PsFragsK<KW> cf;
  load_ps_cell_frags(p, cell0, lane, cf);
  const float ap = p.a_p[cell0 + r], as = p.a_s[cell0 + r];
  // the cell's segment code: -1 for a row beyond B, a negative code and a code the table has no rows for
  int code = -1;
  if (cell0 + r < p.B) {
    code = a.seg ? a.seg[cell0 + r] : 0;
    if (code >= a.n_seg) code = -1;
  }
  if (tid < 32) s_seg[tid] = code;
  const bool cell_ok = code >= 0;
  const int cell_id = a.cell_ids ? a.cell_ids[min(cell0 + r, p.B - 1)] : cell0 + r;
  NbStream st{{(unsigned)a.key, (unsigned)(a.key >> 32)}, 0u, (unsigned)cell_id, a.sample};
  __syncthreads();
  const int ntiles = (a.n_genes + 31) >> 5;
  const bf16_t* const wm_hi = nbs_in_vgpr(a.Wm_hi), * const wm_lo = NSPLIT == 3 ? nbs_in_vgpr(a.Wm_lo) : nullptr;
  const int* const genes = a.genes ? nbs_in_vgpr(a.genes) : nullptr;
  const float* const theta = nbs_in_vgpr(a.theta);
  u64_t* const stats = nbs_in_vgpr(a.stats);
  int* const tile = s_t[wave];
  const bf16_t* const arow = s_am + r * DX_APITCH + 8 * h;
  u64_t total = 0;   // the lane's cell, the lane's half of every tile's genes
  for (int t = blockIdx.y * 4 + wave; t < ntiles; t += gridDim.y * 4) {
    const int sel0 = t * 32;
    const int g = dx_tile_gene(genes, a.n_genes, sel0, r, p.G);   // (a column beyond the selection: never drawn, never counted)
    if (h == 0) { s_gid[wave][r] = g; s_th[wave][r] = theta[g]; }
    f16v yp, ys, acc;
    dx_decode_tile<NSPLIT, KW>(wps_hi, wps_lo, wm_hi, wm_lo, a.K, g, h, arow, cf, yp, ys, acc);
    dx_wave_sync();   // s_gid / s_th of this tile are visible to the wave
    // ---- draws (lane-divergent from here to the hand-over) -> the wave's LDS tile [cell r][gene crow(q, h)] ------------------
#pragma clang loop unroll(disable)
    for (int q = 0; q < 16; ++q) {
      const int gc = crow(q, h);
      if (cell_ok && sel0 + gc < a.n_genes) {
        st.gene = (unsigned)s_gid[wave][gc];
        const int x = nbmix_draw(st, __expf(yp[0] + ap), __expf(ys[0] + as), s_th[wave][gc], acc[0]);
        tile[r * DX_TPITCH + gc] = x;
        total += (unsigned)x;
      }
      yp = nbs_rot(yp); ys = nbs_rot(ys); acc = nbs_rot(acc);
    }
    dx_wave_sync();
    // ---- reduce with lane = gene: cells h, h + 2, ... of the tile, one pending (segment, four values) per half -------------------
    const int col = sel0 + r;
    const bool col_ok = col < a.n_genes;
    int cur = -1;
    u64_t s = 0, sq = 0;
    unsigned nz = 0, mx = 0;
#pragma clang loop unroll(disable)
    for (int c = h; c < 32; c += 2) {
      const int sg = s_seg[c];
      if (sg < 0) continue;   // not drawn: the tile holds an older value there
      if (sg != cur) {
        if (col_ok) dss_flush(stats, a.ld_stats, cur, col, s, nz, sq, mx);
        cur = sg; s = 0; sq = 0; nz = 0; mx = 0;
      }
      const unsigned x = col_ok ? (unsigned)tile[c * DX_TPITCH + r] : 0u;   // (draws are >= 0)
      s += x; sq += (u64_t)x * x; nz += x != 0u; mx = max(mx, x);
    }
    // the wave is whole again: lanes r and r + 32 hold the two halves of gene r; one flush for both when they end in one segment
    {
      const int ocur = __shfl_xor(cur, 32);
      const u64_t os = __shfl_xor(s, 32), osq = __shfl_xor(sq, 32);
      const unsigned onz = __shfl_xor(nz, 32), omx = __shfl_xor(mx, 32);
      if (ocur == cur) {
        if (h == 0) { s += os; sq += osq; nz += onz; mx = max(mx, omx); }
        else s = 0;
      }
    }
    if (col_ok) dss_flush(stats, a.ld_stats, cur, col, s, nz, sq, mx);
    dx_wave_sync();   // the tile and the gene rows are rewritten by the next iteration
  }
  if (cell_ok && a.cell_total) atomicAdd(a.cell_total + cell0 + r, total);
}

}  // namespace spv
