// The fp64 Gram of an fp32 block (spv_gram_f64; spVIPES.get_feature_correlation_matrix of the user API): over the counted rows r of x
//
//   sums[j]    += sum_r (double) x[r][j]                      gram[i][j] += sum_r (double) x[r][i] * (double) x[r][j]
//
// Every x is widened to fp64 first, so every product is exact (two 24-bit significands give 48 bits, fp64 keeps 53): the tables carry
// summation error only, which is what lets the host subtract S S^T / n from C afterwards (data.correlation_table).
//
// How the work is laid out on the chip.  The table is cut into 64 x 64 tiles and only the tiles of the UPPER triangle (tile row <= tile
// column) are computed; the counted rows are cut into `slabs` runs of `per` rows (gram_slabs / gram_slab_rows, pure functions of (n, n_use)).
// One workgroup of four waves owns one (tile, slab): grid (triangle tiles, slabs), 256 threads.
//   * A chunk of GRAM_KC = 32 rows is staged in LDS, already widened, as two panels of 64 columns: the genes of the tile row (panel I)
//     and of the tile column (panel J; on a diagonal tile it IS panel I and is neither loaded nor stored).  The next chunk's global loads
//     are issued before the current chunk's MFMAs (2048 cycles of them per wave, which is what hides the loads' latency) and wait in
//     sixteen fp32 registers.  Rows come through `rows` (clamped into the block: a wrong row number reads a wrong row, never
//     outside x); a row past the slab's end or a column >= n stages +0 and is NOT read (gram_load / gram_counts).
//   * Wave (wr, wc) owns the 32 x 32 quadrant (wr, wc) of the tile as 2 x 2 fragments of v_mfma_f64_16x16x4_f64, 4 doubles per lane each
//     (32 VGPRs of accumulators).  A K step is 4 rows: lane l supplies A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15], ONE double
//     each, so both operands are the same lane map on the staged panel, element [4 ks + (l >> 4)][16 f + (l & 15)] (gram_operand).
//     Two A and two B reads feed four MFMAs.  Rows are fed in ascending order.
//   * The result map is the f64 one, NOT the map of every other MFMA in this library: register `reg` of lane l is
//     row (l >> 4) + 4 * reg, column l & 15 of the fragment (gram_result_row / gram_result_col).
//   * The instruction takes 16 passes (64 cycles) for 1024 multiply-adds, and four of them need four 8-byte LDS reads per lane, so the
//     LDS panels are not double buffered.  Measured, the kernel reaches 36 % of the fp64 matrix peak at 4096 rows x 2048 columns, where
//     the MFMAs alone would allow about twice that; DESIGN.md section 26 has the numbers and what was not tried.
//   * On a diagonal tile the wave below the diagonal (wr = 1, wc = 0) issues no MFMA, and wave 0 adds the panel's columns, one column
//     per lane in ascending row order, for `sums`.
// Writing.  One slab: the owner adds its accumulator onto gram[i][j] for i <= j and the SAME accumulator onto the mirror gram[j][i] for
// i < j (gram_add) -- on diagonal tiles too, where the fragments below the diagonal are computed and dropped.  Each element of the table
// has one writer, so a table that starts symmetric in bits ends symmetric in bits.  More slabs: every workgroup stores its whole tile to
// ws[slab][tile][64 * 64] and its column sums to the tail of ws, and gram_merge_kernel (same ABI call, grid (tiles, 16), one element per
// thread) adds the slabs in ascending slab order from +0 (gram_merge), then does the one add onto the tables.  No floating-point
// atomics, every order fixed: two calls on the same (n, n_use) agree bit for bit.
// Never touched: columns >= n of gram's rows, ws beyond gram_ws_bytes, rows outside `rows`, columns >= n of x (they may hold NaN).
//
// Resources (what the compiler reports with the build's flags; DESIGN.md section 26 has the table): no scratch, no spills, 40 960 bytes
// of LDS.  Kernel rules as for the likelihood and read-out kernels: fixed trip counts inside a chunk, barriers only in uniform code.
//
// The part between the two GRAM-CORE marks is plain C++ apart from __host__ __device__: tools/gram_host_check.py compiles exactly that
// text for the CPU, emulates the 256 threads around it with a plain loop in place of the MFMA, and compares whole tables with numpy.
#pragma once
#include "spv_common.h"

namespace spv {

// ---- GRAM-CORE-BEGIN ----
constexpr int GRAM_MAX_N = 4096;        // SPV_GRAM_MAX_N
constexpr int GRAM_T = 64;              // tile edge
constexpr int GRAM_KC = 32;             // rows staged per chunk: eight K steps of the MFMA
constexpr int GRAM_LDP = 80;            // doubles per staged panel row: 64 + 16, so consecutive rows start half the LDS banks apart
constexpr int GRAM_PANEL = GRAM_KC * GRAM_LDP;
constexpr int GRAM_THREADS = 256;
constexpr int GRAM_TARGET_WG = 512;     // the slab plan aims at this many workgroups
constexpr int GRAM_SLAB_MIN_ROWS = 32;  // ... with at least this many rows per slab
constexpr int GRAM_SLAB_MAX = 128;

__host__ __device__ __forceinline__ int gram_tiles(int n) { return (n + GRAM_T - 1) / GRAM_T; }
__host__ __device__ __forceinline__ int gram_tri_tiles(int nt) { return nt * (nt + 1) / 2; }

// triangle index t in [0, nt (nt + 1) / 2) -> (tile row ti, tile column tj >= ti): row ti holds the nt - ti tiles (ti, ti) .. (ti, nt - 1)
__host__ __device__ __forceinline__ void gram_tile_of(int t, int nt, int& ti, int& tj) {
  ti = 0;
  while (ti < nt - 1 && t >= nt - ti) { t -= nt - ti; ++ti; }
  tj = ti + t;
}

// row slabs of a call: a pure function of (n, n_use).  Enough of them that a few dozen genes still fill the chip, never so many that a
// slab has fewer than GRAM_SLAB_MIN_ROWS rows, and one as soon as the triangle alone has GRAM_TARGET_WG tiles (n >= 1985): slabs * tiles
// stays below 2 * GRAM_TARGET_WG, which bounds the workspace (gram_ws_bytes) by 1022 tiles of 32 KiB, under 32 MiB.
inline int gram_slabs(int n, int n_use) {
  if (n < 1 || n > GRAM_MAX_N || n_use < 1) return 1;
  const int tiles = gram_tri_tiles(gram_tiles(n));
  if (tiles >= GRAM_TARGET_WG) return 1;
  int s = (GRAM_TARGET_WG + tiles - 1) / tiles;
  const int most = n_use / GRAM_SLAB_MIN_ROWS;
  if (s > most) s = most;
  if (s > GRAM_SLAB_MAX) s = GRAM_SLAB_MAX;
  return s < 1 ? 1 : s;
}
// rows per slab, a multiple of the chunk: slab s counts the rows [s * per, min((s + 1) * per, n_use)) of the counted sequence (the last
// slabs may come out empty; they add +0)
__host__ __device__ __forceinline__ int gram_slab_rows(int n_use, int slabs) {
  const int per = (n_use + slabs - 1) / slabs;
  return (per + GRAM_KC - 1) / GRAM_KC * GRAM_KC;
}
// doubles of [slabs][tiles][64 * 64] partial tiles followed by [slabs][nt * 64] partial column sums; nothing for one slab
inline long long gram_ws_doubles(int n, int slabs) {
  if (n < 1 || n > GRAM_MAX_N || slabs <= 1) return 0;
  const int nt = gram_tiles(n);
  return (long long)slabs * ((long long)gram_tri_tiles(nt) * GRAM_T * GRAM_T + (long long)nt * GRAM_T);
}
inline long long gram_ws_bytes(int n, int n_use) { return gram_ws_doubles(n, gram_slabs(n, n_use)) * 8; }
__host__ __device__ __forceinline__ long gram_ws_tile(int slab, int tile, int tiles) { return ((long)slab * tiles + tile) * (GRAM_T * GRAM_T); }
__host__ __device__ __forceinline__ long gram_ws_sums(int slab, int slabs, int nt, int tiles) {
  return (long)slabs * tiles * (GRAM_T * GRAM_T) + (long)slab * nt * GRAM_T;
}

// staging: thread t of the 256 fills column gram_stage_col(t) of panel gram_stage_panel(t), rows gram_stage_row(t, m), m = 0 .. 15
__host__ __device__ __forceinline__ int gram_stage_panel(int t) { return (t >> 6) & 1; }
__host__ __device__ __forceinline__ int gram_stage_col(int t) { return t & 63; }
__host__ __device__ __forceinline__ int gram_stage_row(int t, int m) { return (t >> 7) + 2 * m; }
// whether counted row r (of [.., r_hi), r_hi >= 1) and column c take part: what does not is staged as +0
__host__ __device__ __forceinline__ bool gram_counts(int r, int r_hi, int c, int n) { return r < r_hi && c < n; }
// what the stage loads for (r, c): ALWAYS an element of a counted row and of a column < n.  An (r, c) that does not count loads the
// nearest element that does and its value is dropped at staging (gram_counts), so the load has no branch to wait in -- a guarded load made
// the compiler wait for each of a chunk's loads in turn -- and still nothing outside the counted part of x is ever read.
// Two steps, so that a chunk's row numbers are all asked for before the first of them is needed: the row of x, then the element.
__host__ __device__ __forceinline__ int gram_source_row(const int* rows, int n_rows, int r, int r_hi) {
  const int rr = r < r_hi ? r : r_hi - 1;
  const int src = rows ? rows[rr] : rr;
  return src < 0 ? 0 : (src >= n_rows ? n_rows - 1 : src);
}
__host__ __device__ __forceinline__ float gram_load(const float* x, long ld_x, int src, int c, int n) { return x[(long)src * ld_x + (c < n ? c : n - 1)]; }

// the MFMA's operand of lane l in K step ks (rows 4 ks .. 4 ks + 3 of the chunk) for the fragment at columns `col0` of a panel:
// A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15] are the same element of the staged rows
__host__ __device__ __forceinline__ int gram_operand(int lane, int ks, int col0) { return (4 * ks + (lane >> 4)) * GRAM_LDP + col0 + (lane & 15); }
// the MFMA's result register `reg` (0 .. 3) of lane l within its 16 x 16 fragment: the f64 map
__host__ __device__ __forceinline__ int gram_result_row(int lane, int reg) { return (lane >> 4) + 4 * reg; }
__host__ __device__ __forceinline__ int gram_result_col(int lane) { return lane & 15; }
// the wave's quadrant of the tile and whether it has anything above or on the diagonal
__host__ __device__ __forceinline__ int gram_wave_row(int wave) { return wave >> 1; }
__host__ __device__ __forceinline__ int gram_wave_col(int wave) { return wave & 1; }
__host__ __device__ __forceinline__ bool gram_wave_works(int wave, bool diag) { return !(diag && gram_wave_row(wave) > gram_wave_col(wave)); }

// the one add onto the table: element (i, j) of the upper triangle and its mirror take the same `v`
__host__ __device__ __forceinline__ void gram_add(double* gram, long ld_gram, int n, int i, int j, double v) {
  if (i >= n || j >= n || i > j) return;
  gram[(long)i * ld_gram + j] += v;
  if (i != j) gram[(long)j * ld_gram + i] += v;
}
// the slabs' partial values of one element, `st` apart, added in slab order from +0
__host__ __device__ __forceinline__ double gram_merge(const double* part, long st, int slabs) {
  double sum = 0.0;
#pragma unroll 8
  for (int s = 0; s < slabs; ++s) sum += part[s * st];   // (unrolled: eight loads in flight, the adds in slab order all the same)
  return sum;
}
// ---- GRAM-CORE-END ----

typedef __attribute__((ext_vector_type(4))) double d4v;

struct GramArgs {
  const float* x; long ld_x; int n_rows;
  const int* rows; int n_use;
  int n;
  double* sums;
  double* gram; long ld_gram;
  double* ws;
  int slabs, per, nt, tiles;
};

// grid (tiles, slabs), GRAM_THREADS threads, 2 * GRAM_PANEL doubles of LDS
__global__ __launch_bounds__(GRAM_THREADS) void gram_partial_kernel(const GramArgs a) {
  __shared__ __align__(16) double panels[2 * GRAM_PANEL];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int ti, tj;
  gram_tile_of(blockIdx.x, a.nt, ti, tj);
  const bool diag = ti == tj;
  const int slab = blockIdx.y;
  const int r_lo = slab * a.per;
  const int r_hi = r_lo + a.per < a.n_use ? r_lo + a.per : a.n_use;
  const int chunks = r_hi > r_lo ? (r_hi - r_lo + GRAM_KC - 1) / GRAM_KC : 0;

  const int s_panel = gram_stage_panel(tid), s_col = gram_stage_col(tid);
  const bool stages = !(diag && s_panel);   // the same for a whole wave
  const int s_gcol = (s_panel ? tj : ti) * GRAM_T + s_col;
  double* const s_dst = panels + s_panel * GRAM_PANEL + s_col;
  const double* const pI = panels;
  const double* const pJ = diag ? panels : panels + GRAM_PANEL;
  const int wr = gram_wave_row(wave), wc = gram_wave_col(wave);
  const bool works = gram_wave_works(wave, diag);
  const bool adds_columns = diag && wave == 0;

  d4v acc[2][2];
#pragma unroll
  for (int fi = 0; fi < 2; ++fi)
#pragma unroll
    for (int fj = 0; fj < 2; ++fj) acc[fi][fj] = d4v{0.0, 0.0, 0.0, 0.0};
  double colsum = 0.0;

  float v[GRAM_KC / 2];
  int src[GRAM_KC / 2];
  if (stages) {
#pragma unroll
    for (int m = 0; m < GRAM_KC / 2; ++m) src[m] = gram_source_row(a.rows, a.n_rows, r_lo + gram_stage_row(tid, m), r_hi);
#pragma unroll
    for (int m = 0; m < GRAM_KC / 2; ++m) v[m] = gram_load(a.x, a.ld_x, src[m], s_gcol, a.n);
  }

  for (int c = 0; c < chunks; ++c) {
    const int r_now = r_lo + c * GRAM_KC, r_next = r_now + GRAM_KC;
    if (stages) {
#pragma unroll
      for (int m = 0; m < GRAM_KC / 2; ++m)
        s_dst[gram_stage_row(tid, m) * GRAM_LDP] = gram_counts(r_now + gram_stage_row(tid, m), r_hi, s_gcol, a.n) ? (double)v[m] : 0.0;
    }
    __syncthreads();
    if (stages) {   // the next chunk's loads; after the last chunk they repeat the slab's last row and are dropped
#pragma unroll
      for (int m = 0; m < GRAM_KC / 2; ++m) src[m] = gram_source_row(a.rows, a.n_rows, r_next + gram_stage_row(tid, m), r_hi);
#pragma unroll
      for (int m = 0; m < GRAM_KC / 2; ++m) v[m] = gram_load(a.x, a.ld_x, src[m], s_gcol, a.n);
    }
    if (works) {
#pragma unroll
      for (int ks = 0; ks < GRAM_KC / 4; ++ks) {
        const double a0 = pI[gram_operand(lane, ks, 32 * wr)], a1 = pI[gram_operand(lane, ks, 32 * wr + 16)];
        const double b0 = pJ[gram_operand(lane, ks, 32 * wc)], b1 = pJ[gram_operand(lane, ks, 32 * wc + 16)];
        acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
      }
    }
    if (adds_columns) {
#pragma unroll
      for (int r = 0; r < GRAM_KC; ++r) colsum += pI[r * GRAM_LDP + lane];
    }
    __syncthreads();
  }

  const bool direct = a.slabs == 1;
  double* const part = direct ? nullptr : a.ws + gram_ws_tile(slab, blockIdx.x, a.tiles);
#pragma unroll
  for (int fi = 0; fi < 2; ++fi)
#pragma unroll
    for (int fj = 0; fj < 2; ++fj)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int lr = 32 * wr + 16 * fi + gram_result_row(lane, reg), lc = 32 * wc + 16 * fj + gram_result_col(lane);
        if (direct) gram_add(a.gram, a.ld_gram, a.n, ti * GRAM_T + lr, tj * GRAM_T + lc, acc[fi][fj][reg]);
        else part[lr * GRAM_T + lc] = acc[fi][fj][reg];
      }
  if (adds_columns) {
    const int j = ti * GRAM_T + lane;
    if (direct) { if (j < a.n) a.sums[j] += colsum; }
    else a.ws[gram_ws_sums(slab, a.slabs, a.nt, a.tiles) + j] = colsum;
  }
}

// grid (tiles, 64 * 64 / GRAM_THREADS), GRAM_THREADS threads, one element of the tile per thread: the slabs' partial tiles and column sums
// in slab order, then the one add onto the tables
__global__ __launch_bounds__(GRAM_THREADS) void gram_merge_kernel(const GramArgs a) {
  const int tid = threadIdx.x;
  int ti, tj;
  gram_tile_of(blockIdx.x, a.nt, ti, tj);
  const long st = (long)a.tiles * (GRAM_T * GRAM_T);
  const double* const part = a.ws + gram_ws_tile(0, blockIdx.x, a.tiles);
  const int e = tid + GRAM_THREADS * blockIdx.y, lr = e >> 6, lc = e & 63;
  const int i = ti * GRAM_T + lr, j = tj * GRAM_T + lc;
  if (i < a.n && j < a.n && i <= j) gram_add(a.gram, a.ld_gram, a.n, i, j, gram_merge(part + e, st, a.slabs));
  if (ti == tj && blockIdx.y == 0 && tid < GRAM_T) {
    const int j = ti * GRAM_T + tid;
    if (j < a.n) a.sums[j] += gram_merge(a.ws + gram_ws_sums(0, a.slabs, a.nt, a.tiles) + j, (long)a.nt * GRAM_T, a.slabs);
  }
}

}  // namespace spv
