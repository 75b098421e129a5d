// PCA of the log-normalised OBSERVED counts (spVIPES.count_pca / spVIPES.pca of the user API): the two skinny products of a block
// Krylov step against a tall matrix X [n positions][G genes] that is never stored,
//
//   project   Y[p][t]  = sum_j x(p, j) V[j][t]          back   Z[j][t] += sum_p x(p, j) Y[p][t]          (t < l, l in {16, 32, 48, 64})
//
// and the stage that writes x itself (the moments pass of pca_ops.lognorm_moments, and the tests' window on the operand).
//
// The operand, one device function for all three kernels (pca_operand): with c the count of gene j in the cell of list position p,
//   u = (float) c * w[p]         ONE fp32 multiply, never contracted: spv_rank_stage's key ((float) c without w)
//   a = pca_log1p(u)             a fixed sequence of fp32 operations (no library log), a == 0 exactly for u == 0
//   x = (a - mu[j]) * scale[j]   an fp32 subtract, then an fp32 multiply, not fused (mu == NULL: 0, scale == NULL: 1)
// A gene with scale 0 contributes exactly 0 to both products: a gene selection is a scale vector, no column is gathered.
// The products run on v_mfma_f32_32x32x2_f32: every product of two fp32 operands is exact in the fused multiply-add, the sums are fp32
// chains in ascending k, one rounding per term.
//
// How the work is laid out on the chip (PCA_THREADS = 256 threads = four waves in every kernel)
//   * stage: one workgroup per PCA_ST_P list positions x 256 genes, a thread per gene, plain stores.
//   * project: one workgroup owns PCA_CELL_TILE = 64 list positions and walks the genes in ascending tiles of PCA_KT = 32.  A tile of x
//     is made in registers (the counts of the NEXT tile are loaded before the current tile's MFMAs and wait there), goes through the
//     VALU (weight, log1p, centre, scale) and into LDS k-major, xs[gene][cell]; V's tile goes into vs[gene][column], columns >= l as +0.
//     Nine counts in ten are zero, and for a zero count pca_operand gives the gene's constant (0 - mu) * scale: every slot is filled
//     with that constant, each wave lists the non-zero counts of its own 512 slots in LDS (a ballot and a popcount per row of
//     elements, no shared counter) and then runs pca_operand on the list, one lane per listed element.  The values are pca_operand's
//     either way; a matrix without zeros takes eight passes per tile.  What bounds the kernel is not the VALU and not the MFMA but
//     the latency chain of a tile (load, stage, barrier, sixteen MFMAs, barrier) and how many workgroups overlap it: launch a list
//     whole, not in pieces of one workgroup per CU (DESIGN.md section 29 has the measurements).
//     Wave (rb, cb) = (wave & 1, wave >> 1) owns the 32 x 32 block of cells 32 rb .. and columns 32 cb ..: lane (r = lane & 31, h = lane >> 5)
//     feeds A[i = r][k = h] = xs[2 ks + h][32 rb + r] and B[k = h][j = r] = vs[2 ks + h][32 cb + r], sixteen MFMAs per tile into ONE
//     accumulator of sixteen registers.  A wave whose columns all lie at or beyond l issues none.  The sum of a row runs over the genes
//     in ascending order whatever the piece, the tile or the other rows hold: a row's result depends on that row alone.
//   * back: the list is cut into slabs at ABSOLUTE positions, multiples of PCA_SLAB; one workgroup owns 64 genes and one slab and
//     walks the slab's positions in ascending tiles of 32: xs[position][gene], ys[position][column], wave (gb, cb) the block of genes
//     32 gb .. x columns 32 cb .., A[i = r][k = h] = xs[2 ks + h][32 gb + r], B[k = h][j = r] = ys[2 ks + h][32 cb + r].  A position at or
//     beyond the piece's end stages +0 in both panels.  The fp32 partial tile goes to ws[slab of the piece][gene][column] (plain stores,
//     one writer per element), and pca_merge_kernel adds the slabs onto Z in ascending slab order, ONE fp64 addition per slab:
//     Z = (((Z + s0) + s1) + ...).  Slabs are absolute and the merge is sequential, so a list passed in one piece or in many
//     slab-aligned pieces gives the same bits, and two groups' calls collect in one Z.
//
// Every index bound
//   * the list: a slot at or beyond p_end = pos_off + n_piece (<= n, the wrapper checks) reads position p_end - 1 instead and is
//     discarded; rows is read at q - pos_off in [0, n_piece), w at q < n.
//   * the matrix: a row number outside [0, n_rows) and a gene >= G read as a zero count and are never dereferenced: the load goes to
//     row 0 / gene 0 instead, which exist (n_rows > 0, G > 0), and its value is dropped (pca_source); ld >= col_off + G is checked.
//   * mu, scale, V rows and Z rows are indexed by a gene < G only, V / Y / Z columns by t < l <= ld; block by (p - pos_off) < n_piece and
//     j < G <= ld_block; Y rows by p < p_end <= n.
//   * ws: ((slab of the piece) * Gp + gene) * l + t with slab < pca_slabs(n_piece), gene < Gp = round_up(G, 64), t < l: below
//     pca_ws_floats(G, n_piece, l), which the wrapper holds ws_bytes against.
//
// The part between the two PCA-CORE marks is plain C++ apart from __host__ __device__: tools/pca_host_check.py compiles exactly that text
// for the CPU, emulates the workgroups around it with a plain loop in place of the MFMA, and compares with numpy.
#pragma once
#include "spv_common.h"
#include <cmath>

namespace spv {

// ---- PCA-CORE-BEGIN ----
constexpr int PCA_THREADS = 256;
constexpr int PCA_CELL_TILE = 64;   // project: list positions per workgroup           (spv_pca_cell_tile())
constexpr int PCA_SLAB = 1024;      // back: list positions per slab, absolute bounds   (spv_pca_slab(); divides COUNT_CHUNK_ROWS = 4096)
constexpr int PCA_GENE_TILE = 64;   // back: genes per workgroup
constexpr int PCA_KT = 32;          // contraction tile of both products: sixteen K steps of the MFMA
constexpr int PCA_LMAX = 64;        // columns, at most
constexpr int PCA_LDX = 66;         // project: floats per xs row (64 cells + 2: a wave's two cells of 32 genes fall into 64 banks)
constexpr int PCA_LDV = 96;         // floats per vs / ys / back-xs row (64 + 32: a lane half's 32 words start half the banks apart)
constexpr int PCA_ST_P = 8;         // stage: list positions per workgroup

// l is one of 16, 32, 48, 64
__host__ __device__ __forceinline__ bool pca_l_ok(int l) { return l == 16 || l == 32 || l == 48 || l == 64; }

// the slab plan: slab s holds the absolute positions [s * PCA_SLAB, (s + 1) * PCA_SLAB); a piece starts on a slab bound
__host__ __device__ __forceinline__ int pca_slabs(int n_piece) { return (n_piece + PCA_SLAB - 1) / PCA_SLAB; }
__host__ __device__ __forceinline__ int pca_gene_pad(int G) { return (G + PCA_GENE_TILE - 1) / PCA_GENE_TILE * PCA_GENE_TILE; }
// fp32 partial tiles [slabs of the piece][Gp][l]
inline long long pca_ws_floats(int G, int n_piece, int l) {
  if (G < 1 || n_piece < 1 || !pca_l_ok(l)) return 0;
  return (long long)pca_slabs(n_piece) * pca_gene_pad(G) * l;
}
inline long long pca_ws_bytes(int G, int n_piece, int l) { return pca_ws_floats(G, n_piece, l) * 4; }
__host__ __device__ __forceinline__ long pca_ws_at(int slab, int Gp, int gene, int l, int t) { return ((long)slab * Gp + gene) * l + t; }

// the list position a slot reads (a position of the piece that exists: n_piece > 0) and the element a lane loads: the cell's own when it
// counts, else row 0 / gene 0 (n_rows > 0, ld >= col_off + G > col_off)
__host__ __device__ __forceinline__ int pca_position(int p, int p_end) { return p < p_end ? p : p_end - 1; }
__host__ __device__ __forceinline__ long pca_source(bool counts, int row, long ld, int col_off, int gene) {
  return (long)(counts ? row : 0) * ld + col_off + (counts ? gene : 0);
}

// staging maps, thread t of the 256.  project: gene pca_pj_gene(t) of the K tile, cells pca_pj_cell(t, m), m = 0 .. 7; V's tile: column
// pca_col(t), K rows pca_k4(t, m).  back: gene pca_col(t) of the gene tile, positions pca_k4(t, m) of the K tile, the same for ys.
__host__ __device__ __forceinline__ int pca_pj_gene(int t) { return t & 31; }
__host__ __device__ __forceinline__ int pca_pj_cell(int t, int m) { return (t >> 5) + 8 * m; }
__host__ __device__ __forceinline__ int pca_col(int t) { return t & 63; }
__host__ __device__ __forceinline__ int pca_k4(int t, int m) { return (t >> 6) + 4 * m; }
// the MFMA's operands of lane `lane` in K step ks of a tile staged k-major with `ldp` floats per row, for the block at `m0`:
// A[i = lane & 31][k = lane >> 5] and B[k = lane >> 5][j = lane & 31] are the same map
__host__ __device__ __forceinline__ int pca_operand_at(int lane, int ks, int m0, int ldp) { return (2 * ks + (lane >> 5)) * ldp + m0 + (lane & 31); }
// the result register `reg` (0 .. 15) of lane `lane` within its 32 x 32 block
__host__ __device__ __forceinline__ int pca_result_row(int lane, int reg) { return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5); }
__host__ __device__ __forceinline__ int pca_result_col(int lane) { return lane & 31; }
__host__ __device__ __forceinline__ int pca_wave_lo(int wave) { return wave & 1; }    // the block along cells (project) / genes (back)
__host__ __device__ __forceinline__ int pca_wave_col(int wave) { return wave >> 1; }  // the block along the l columns

// log(1 + u) for u >= 0 in fp32 operations only, the same bits on every machine that rounds to nearest: t = fl(1 + u) with its
// rounding error c recovered exactly, log t by the argument reduction t = m 2^e, m in [sqrt(1/2), sqrt 2), and the minimax polynomial
// of s = f / (2 + f), f = m - 1 (the classic single-precision log kernel), plus c / t.  u == 0 (and anything that is not > 0) gives 0.
__host__ __device__ __forceinline__ float pca_log1p(float u) {
#pragma clang fp contract(off)
  if (!(u > 0.f)) return 0.f;
  const float t = 1.f + u;
  const float c = u < 1.f ? u - (t - 1.f) : 1.f - (t - u);
  int e;
  float m = frexpf(t, &e);                       // t = m 2^e, m in [1/2, 1)
  if (m < 0.70710678f) { m = m + m; e -= 1; }
  const float f = m - 1.f;
  const float s = f / (2.f + f);
  const float z = s * s, w = z * z;
  const float t1 = w * (0.40000972152f + w * 0.24279078841f);
  const float t2 = z * (0.66666662693f + w * 0.28498786688f);
  const float r = t2 + t1;
  const float hfsq = 0.5f * f * f;
  const float dk = (float)e;
  const float lg = dk * 6.9313812256e-01f - ((hfsq - (s * (hfsq + r) + dk * 9.0580006145e-06f)) - f);
  return lg + c / t;
}
// x(p, j): weight, log1p, centre, scale -- four roundings, none of them fused with a neighbour
__host__ __device__ __forceinline__ float pca_operand(float c, float w, bool has_w, float mu, float scale) {
#pragma clang fp contract(off)
  const float u = has_w ? c * w : c;
  const float a = pca_log1p(u);
  const float d = a - mu;
  return d * scale;
}

// the slabs' partial values of one element, `st` floats apart, added onto z in slab order, one fp64 addition each
__host__ __device__ __forceinline__ double pca_merge(double z, const float* part, long st, int slabs) {
  for (int s = 0; s < slabs; ++s) z += (double)part[s * st];
  return z;
}
// ---- PCA-CORE-END ----

typedef __attribute__((ext_vector_type(16))) float pca_acc_t;
constexpr int PCA_WAVE_ELEMS = PCA_KT * 64 / 4;   // elements of a tile that one wave stages: 512

struct PcaArgs {
  const void* X; long ld; const int* rows; int col_off;   // the matrix; list position p -> rows[p - pos_off] (nullptr: p - pos_off)
  int G, n_rows, n_piece, pos_off, n, l;
  const float* w; const float* mu; const float* scale;
  float* block; long ld_block;
  const float* V; long ld_v;
  float* Y; long ld_y;
  double* Z; long ld_z;
  float* ws;
};

template <bool U16>
__device__ __forceinline__ float pca_count(const void* X, long at) {
  if constexpr (U16) return (float)reinterpret_cast<const unsigned short*>(X)[at];
  else return reinterpret_cast<const float*>(X)[at];
}

// grid (ceil(n_piece / PCA_ST_P), ceil(G / 256)): block[p - pos_off][j] = x(p, j)
template <bool U16>
__global__ __launch_bounds__(PCA_THREADS) void pca_stage_kernel(const PcaArgs a) {
  const int j = (int)blockIdx.y * PCA_THREADS + (int)threadIdx.x;
  const bool g_ok = j < a.G;
  const int p_end = a.pos_off + a.n_piece;
  const float mu = (a.mu && g_ok) ? a.mu[j] : 0.f, sc = (a.scale && g_ok) ? a.scale[j] : 1.f;
#pragma unroll
  for (int i = 0; i < PCA_ST_P; ++i) {
    const int p = a.pos_off + (int)blockIdx.x * PCA_ST_P + i;
    const int q = pca_position(p, p_end);
    const int r = a.rows ? a.rows[q - a.pos_off] : q - a.pos_off;
    const bool ok = g_ok && r >= 0 && r < a.n_rows;
    const float c = pca_count<U16>(a.X, pca_source(ok, r, a.ld, a.col_off, j));
    const float wv = a.w ? a.w[q] : 1.f;
    if (p < p_end && g_ok) a.block[(long)(p - a.pos_off) * a.ld_block + j] = pca_operand(ok ? c : 0.f, wv, a.w != nullptr, mu, sc);
  }
}

// grid (ceil(n_piece / PCA_CELL_TILE)): Y[p][t] = sum_j x(p, j) V[j][t]
template <bool U16>
__global__ __launch_bounds__(PCA_THREADS) void pca_project_kernel(const PcaArgs a) {
  __shared__ float xs[PCA_KT * PCA_LDX];
  __shared__ float vs[PCA_KT * PCA_LDV];
  __shared__ float wl[PCA_CELL_TILE];                      // the tile's cell weights
  __shared__ float mus[4][PCA_KT], scs[4][PCA_KT];         // per wave: mu and scale of the K tile's genes
  __shared__ int li[4][PCA_WAVE_ELEMS];                    // per wave: the non-zero counts of its 512 elements of the tile, (gene << 8) | cell ...
  __shared__ float lc[4][PCA_WAVE_ELEMS];                  // ... and the count itself
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  const int p0 = a.pos_off + (int)blockIdx.x * PCA_CELL_TILE, p_end = a.pos_off + a.n_piece;
  const int rb = pca_wave_lo(wave), cb = pca_wave_col(wave);
  const bool works = 32 * cb < a.l;   // (the same for a whole wave)
  const bool has_w = a.w != nullptr;
  // this thread's eight cells: row number, weight, whether the row exists -- fixed for the whole walk
  int row[8];
  float wv[8];
  bool r_ok[8];
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    const int q = pca_position(p0 + pca_pj_cell(tid, m), p_end);
    row[m] = a.rows ? a.rows[q - a.pos_off] : q - a.pos_off;
    r_ok[m] = row[m] >= 0 && row[m] < a.n_rows;
    wv[m] = has_w ? a.w[q] : 1.f;
  }
  const int gl = pca_pj_gene(tid), vc = pca_col(tid);
  const bool vc_ok = vc < a.l;
  if (gl == 0) {
#pragma unroll
    for (int m = 0; m < 8; ++m) wl[pca_pj_cell(tid, m)] = wv[m];
  }
  __syncthreads();

  pca_acc_t acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;

  float c[8], mu = 0.f, sc = 1.f;
  bool g_ok;
  {
    const int j = gl;
    g_ok = j < a.G;
#pragma unroll
    for (int m = 0; m < 8; ++m) c[m] = pca_count<U16>(a.X, pca_source(g_ok && r_ok[m], row[m], a.ld, a.col_off, j));
    mu = (a.mu && g_ok) ? a.mu[j] : 0.f;
    sc = (a.scale && g_ok) ? a.scale[j] : 1.f;
  }
  // V's tile waits in registers a tile ahead as well: a row at or beyond G and a column at or beyond l are +0 and are not read
  float vv[8];
  auto load_v = [&](int j0) {
#pragma unroll
    for (int m = 0; m < 8; ++m) {
      const int j = j0 + pca_k4(tid, m);
      vv[m] = (vc_ok && j < a.G) ? a.V[(long)j * a.ld_v + vc] : 0.f;
    }
  };
  load_v(0);
  const int tiles = (a.G + PCA_KT - 1) / PCA_KT;
  for (int kt = 0; kt < tiles; ++kt) {
    const int j0 = kt * PCA_KT;
    // x of this tile.  A zero count gives the gene's constant x0 = pca_operand(0) = (0 - mu) * scale, whatever the weight: every slot is
    // filled with it (a gene beyond G: +0, as its V rows), and the NON-ZERO counts -- a tenth of single-cell data -- are listed per wave
    // (two ballots' worth of bookkeeping, no shared counter) and go through the operand function afterwards, a lane per listed element.
    // The listed elements are the wave's own 512 slots, so this needs no workgroup barrier; the values are pca_operand's either way.
    {
      const float x0 = g_ok ? pca_operand(0.f, 1.f, false, mu, sc) : 0.f;
      if (lane < PCA_KT) { mus[wave][gl] = mu; scs[wave][gl] = sc; }   // (lanes 0 .. 31 of every wave hold the tile's 32 genes)
      int cnt = 0;
#pragma unroll
      for (int m = 0; m < 8; ++m) {
        const int cell = pca_pj_cell(tid, m);
        xs[gl * PCA_LDX + cell] = x0;
        const bool nz = g_ok && r_ok[m] && c[m] != 0.f;
        const unsigned long long b = __ballot(nz);
        if (nz) {
          const int at = cnt + __builtin_popcountll(b & below);   // < 512: at most one entry per element of the wave
          li[wave][at] = (gl << 8) | cell;
          lc[wave][at] = c[m];
        }
        cnt += __builtin_popcountll(b);
      }
      // The lanes of this wave hand li / lc / mus / scs / xs to each other through LDS with no workgroup barrier and no memory fence.
      // None is needed: the loads below may alias the stores above (the same __shared__ arrays, indices the compiler cannot tell
      // apart), so the compiler must keep their program order; a wave's LDS operations execute in that order; and the compiler's
      // own wait on the LDS counter stands before the first use of a loaded value.  The scheduling barrier only pins the place.  (A
      // fence builtin would say the same; this header stays free of every memory-order builtin, which its ABI test holds it to.)
      __builtin_amdgcn_wave_barrier();
      for (int i = lane; i < cnt; i += 64) {
        const int e = li[wave][i], g = e >> 8, cell = e & 255;
        xs[g * PCA_LDX + cell] = pca_operand(lc[wave][i], has_w ? wl[cell] : 1.f, has_w, mus[wave][g], scs[wave][g]);
      }
    }
#pragma unroll
    for (int m = 0; m < 8; ++m) vs[pca_k4(tid, m) * PCA_LDV + vc] = vv[m];
    __syncthreads();
    load_v(j0 + PCA_KT);
    {   // the next tile's counts; beyond the last tile they repeat gene 0 and are dropped
      const int j = j0 + PCA_KT + gl;
      g_ok = j < a.G;
#pragma unroll
      for (int m = 0; m < 8; ++m) c[m] = pca_count<U16>(a.X, pca_source(g_ok && r_ok[m], row[m], a.ld, a.col_off, j));
      mu = (a.mu && g_ok) ? a.mu[j] : 0.f;
      sc = (a.scale && g_ok) ? a.scale[j] : 1.f;
    }
    if (works) {
#pragma unroll
      for (int ks = 0; ks < PCA_KT / 2; ++ks)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xs[pca_operand_at(lane, ks, 32 * rb, PCA_LDX)], vs[pca_operand_at(lane, ks, 32 * cb, PCA_LDV)], acc, 0, 0, 0);
    }
    __syncthreads();
  }
  if (works) {
    const int t = 32 * cb + pca_result_col(lane);
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int p = p0 + 32 * rb + pca_result_row(lane, reg);
      if (p < p_end && t < a.l) a.Y[(long)p * a.ld_y + t] = acc[reg];
    }
  }
}

// grid (Gp / PCA_GENE_TILE, pca_slabs(n_piece)): ws[slab][gene][t] = sum over the slab's positions of x(p, gene) Y[p][t]
template <bool U16>
__global__ __launch_bounds__(PCA_THREADS) void pca_back_kernel(const PcaArgs a) {
  __shared__ float xs[PCA_KT * PCA_LDV];
  __shared__ float ys[PCA_KT * PCA_LDV];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g0 = (int)blockIdx.x * PCA_GENE_TILE, slab = blockIdx.y;
  const int p_lo = a.pos_off + slab * PCA_SLAB, p_end = a.pos_off + a.n_piece;
  const int p_hi = p_lo + PCA_SLAB < p_end ? p_lo + PCA_SLAB : p_end;
  const int gb = pca_wave_lo(wave), cb = pca_wave_col(wave);
  const bool works = 32 * cb < a.l;
  const bool has_w = a.w != nullptr;
  const int j = g0 + pca_col(tid), vc = pca_col(tid);
  const bool g_ok = j < a.G, vc_ok = vc < a.l;
  const float mu = (a.mu && g_ok) ? a.mu[j] : 0.f, sc = (a.scale && g_ok) ? a.scale[j] : 1.f;

  pca_acc_t acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;

  float c[8], wv[8], yv[8];
  bool ok[8];
  auto load = [&](int pt) {
#pragma unroll
    for (int m = 0; m < 8; ++m) {
      const int p = pt + pca_k4(tid, m);
      const int q = pca_position(p, p_hi);
      const int r = a.rows ? a.rows[q - a.pos_off] : q - a.pos_off;
      ok[m] = g_ok && r >= 0 && r < a.n_rows;
      c[m] = pca_count<U16>(a.X, pca_source(ok[m], r, a.ld, a.col_off, j));
      wv[m] = has_w ? a.w[q] : 1.f;
      yv[m] = a.Y[(long)q * a.ld_y + (vc_ok ? vc : 0)];
    }
  };
  load(p_lo);
  const int tiles = (p_hi - p_lo + PCA_KT - 1) / PCA_KT;
  for (int kt = 0; kt < tiles; ++kt) {
    const int pt = p_lo + kt * PCA_KT;
#pragma unroll
    for (int m = 0; m < 8; ++m) {
      const int k = pca_k4(tid, m);
      const bool live = pt + k < p_hi;
      xs[k * PCA_LDV + pca_col(tid)] = (live && g_ok) ? pca_operand(ok[m] ? c[m] : 0.f, wv[m], has_w, mu, sc) : 0.f;
      ys[k * PCA_LDV + vc] = (live && vc_ok) ? yv[m] : 0.f;
    }
    __syncthreads();
    load(pt + PCA_KT);   // the next tile; beyond the slab's end it repeats the last position and is dropped
    if (works) {
#pragma unroll
      for (int ks = 0; ks < PCA_KT / 2; ++ks)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xs[pca_operand_at(lane, ks, 32 * gb, PCA_LDV)], ys[pca_operand_at(lane, ks, 32 * cb, PCA_LDV)], acc, 0, 0, 0);
    }
    __syncthreads();
  }
  if (works) {
    const int Gp = pca_gene_pad(a.G);
    const int t = 32 * cb + pca_result_col(lane);
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int gene = g0 + 32 * gb + pca_result_row(lane, reg);
      if (t < a.l) a.ws[pca_ws_at(slab, Gp, gene, a.l, t)] = acc[reg];
    }
  }
}

// grid (ceil(G * l / 256)): one element of Z per thread, the piece's slabs in ascending order
__global__ __launch_bounds__(PCA_THREADS) void pca_merge_kernel(const PcaArgs a) {
  const long e = (long)blockIdx.x * PCA_THREADS + threadIdx.x;
  if (e >= (long)a.G * a.l) return;
  const int j = (int)(e / a.l), t = (int)(e % a.l);
  const int Gp = pca_gene_pad(a.G);
  double* const z = a.Z + (long)j * a.ld_z + t;
  *z = pca_merge(*z, a.ws + pca_ws_at(0, Gp, j, a.l, t), (long)Gp * a.l, pca_slabs(a.n_piece));
}

}  // namespace spv
