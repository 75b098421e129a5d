// The rank transform of the column sort (rank_ops.rank_transform; spVIPES.get_feature_spearman_matrix / count_spearman_matrix of the
// user API: Spearman's rho is the Pearson correlation of average ranks, and spv_gram_f64 reads the block this writes).  After the stage
// and the sort of spv_rank.h every list position gets its rank back:
//     out[p * ld_out + j] = (float)(2 * avg_rank(p, j) - (n + 1)) = (float)(L + U - n)
// with L = the keys of gene j smaller than position p's and U = the smaller or equal ones.  An integer in [-(n - 1), n - 1], exact in
// fp32 for n <= 2^20; every column sums to 0 and its squares to (n^3 - n - ties[j]) / 3.
//
// How the work is laid out on the chip
//   * stage: rank_stage_kernel<U16, true> of spv_rank.h -- the low word of an entry is the list position, no segment code is read.
//   * values (rank_values_kernel): one workgroup of RANK_THREADS threads per gene.  The gene owns one fp32 column of n values in a third
//     region of the workspace (gene-major, behind the two halves of the sort).  The workgroup fills the column with the zero run's value
//     n_zero - n (L = 0, U = n_zero), coalesced, unless the gene has no zero key; sorts the stored entries with rank_sort_column (the sort
//     of rank_sums_kernel: its barriers also order the fill before the walk); then entry i of the run [s, e) stores
//     2 n_zero + s + e - n at its own position, a scatter inside the gene's own 4 n bytes.  Every word of the column has ONE writer per
//     phase and the phases are separated by barriers.  The walk uses no atomic: the tie term t^3 - t is summed per thread, per wave by
//     shuffles, and across the waves by thread 0 through RANK_WAVES words of LDS.  (The shared sort keeps the integer LDS atomics of
//     its digit histogram, and the stage its integer cursor; there is no floating-point atomic anywhere.)
//   * store (rank_values_store_kernel): 64 positions x 64 genes per workgroup cross an LDS tile [64][65] (+ 1: a wave reads one position
//     of 64 genes, 65 words apart -> 64 banks): lanes along positions while the columns are read, lanes along genes while the rows of
//     `out` are written, both sides coalesced.
//
// Every index bound
//   * n lies in [1, 2^20] and n_sel in [1, spv_rank_gene_slab()] (the wrappers check both), so j * n + p < 2^30 fits every index type.
//   * stage: the bounds of spv_rank.h.  Rows and genes outside the matrix read as a zero key, from an address that exists (row 0 /
//     gene 0).  The position word of an entry is p < pos_off + n_piece <= n.
//   * values: m = the gene's cursor cut to [0, n], so the sort and the walk stay inside the column's n entries.  The fill writes
//     col[i], i < n.  A position word at or above n (only a caller that breaks the staging contract can make one) is NEVER used as an
//     address: the store is guarded by p < n.  ties[j], nonzero[j]: j < n_sel.
//   * store, reads: a slot of the tile outside the slab or the list reads gene n_sel - 1 / position n - 1 instead, which exist, and is
//     discarded.  Writes: out[p * ld_out + j] only for p < n and j < n_sel <= ld_out: columns at or above n_sel of out are never touched.
#pragma once
#include "spv_rank.h"

namespace spv {

// ---- RANK-VALUES-CORE-BEGIN ----
// (plain C++: tools/spearman_host_check.py compiles this text, behind RANK-CORE of spv_rank.h, for the host)
constexpr int RANKV_T = 64;        // store tile: positions x genes
constexpr int RANKV_THREADS = 256; // threads of a store workgroup: RANKV_T lanes x 4 rows per round

// workspace: [head][half A][half B] of spv_rank.h, then the fp32 columns [n_sel][n]; byte offsets, the total rounded up to 8
__host__ __device__ __forceinline__ long long rank_values_col_off(int n, int n_sel) { return rank_ws_half_off(2, n, n_sel); }
__host__ __device__ __forceinline__ long long rank_values_ws_bytes(int n, int n_sel) {
  if (rank_ws_bytes(n, n_sel) == 0) return 0;
  return (rank_values_col_off(n, n_sel) + 4ll * n * n_sel + 7ll) & ~7ll;
}

// L + U - n: of a zero key (L = 0, U = n_zero); of a stored entry of the run [s, e) above n_zero zero keys
__host__ __device__ __forceinline__ int rank_value_zero(int n_zero, int n) { return n_zero - n; }
__host__ __device__ __forceinline__ int rank_value_term(int n_zero, int s, int e, int n) { return 2 * n_zero + s + e - n; }

// the store's maps: round r of thread t covers row 4 r + t / 64 of the tile with lane t % 64; a slot outside [0, count) reads count - 1;
// element (gene j, position p) of the columns; element (position p, gene j) of out
__host__ __device__ __forceinline__ int rank_tr_row(int r, int t) { return (RANKV_THREADS / RANKV_T) * r + t / RANKV_T; }
__host__ __device__ __forceinline__ int rank_tr_lane(int t) { return t % RANKV_T; }
__host__ __device__ __forceinline__ int rank_tr_clamp(int i, int count) { return i < count ? i : count - 1; }
__host__ __device__ __forceinline__ long rank_tr_src(int j, int p, int n) { return (long)j * n + p; }
__host__ __device__ __forceinline__ long rank_tr_dst(int p, int j, long ld_out) { return (long)p * ld_out + j; }
// ---- RANK-VALUES-CORE-END ----

struct RankValuesArgs {
  int n, n_sel;
  float* out; long ld_out;
  long long* ties; int* nonzero;   // either may be nullptr
  char* ws;
};

__global__ __launch_bounds__(RANK_THREADS) void rank_values_kernel(RankValuesArgs a) {
  __shared__ rank_entry_t buf[RANK_LDS_CAP];
  __shared__ unsigned long long part[RANK_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = blockIdx.x;
  const int* const cursor = reinterpret_cast<const int*>(a.ws + rank_ws_cursor_off());
  const int m = min(max(cursor[j], 0), a.n), n_zero = a.n - m;
  rank_entry_t* const src = reinterpret_cast<rank_entry_t*>(a.ws + rank_ws_half_off(0, a.n, a.n_sel)) + (long)j * a.n;
  rank_entry_t* const dst = reinterpret_cast<rank_entry_t*>(a.ws + rank_ws_half_off(1, a.n, a.n_sel)) + (long)j * a.n;
  float* const col = reinterpret_cast<float*>(a.ws + rank_values_col_off(a.n, a.n_sel)) + (long)j * a.n;
  if (n_zero > 0) {   // (uniform over the workgroup)
    const float z = (float)rank_value_zero(n_zero, a.n);
    for (int i = tid; i < a.n; i += RANK_THREADS) col[i] = z;
  }
  const rank_entry_t* const sorted = rank_sort_column(buf, src, dst, m);   // (ends with a barrier: the fill is behind every thread)
  unsigned long long tie = 0ull;
  for (int i = tid; i < m; i += RANK_THREADS) {
    const int s = rank_run_begin(sorted, i), e = rank_run_end(sorted, i, m);
    const unsigned p = rank_entry_seg(sorted[i]);
    if (p < (unsigned)a.n) col[p] = (float)rank_value_term(n_zero, s, e, a.n);
    if (s == i) tie += rank_tie_term(e - s);
  }
  if (a.ties) {   // (uniform)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const unsigned lo = __shfl_down((unsigned)tie, off, 64), hi = __shfl_down((unsigned)(tie >> 32), off, 64);
      tie += ((unsigned long long)hi << 32) | lo;
    }
    if (lane == 0) part[wave] = tie;
    __syncthreads();
    if (tid == 0) {
      unsigned long long t = rank_tie_term(n_zero);
      for (int w = 0; w < RANK_WAVES; ++w) t += part[w];
      a.ties[j] = (long long)t;
    }
  }
  if (a.nonzero && tid == 0) a.nonzero[j] = m;
}

__global__ __launch_bounds__(RANKV_THREADS) void rank_values_store_kernel(RankValuesArgs a) {
  __shared__ float tile[RANKV_T][RANKV_T + 1];
  const int t = threadIdx.x, p0 = (int)blockIdx.x * RANKV_T, j0 = (int)blockIdx.y * RANKV_T;
  const float* const cols = reinterpret_cast<const float*>(a.ws + rank_values_col_off(a.n, a.n_sel));
  // every load is issued unconditionally, from a slot that exists (rank_tr_clamp); what lies outside is never stored
#pragma unroll
  for (int r = 0; r < RANKV_T * RANKV_T / RANKV_THREADS; ++r) {
    const int gl = rank_tr_row(r, t), pl = rank_tr_lane(t);
    tile[gl][pl] = cols[rank_tr_src(rank_tr_clamp(j0 + gl, a.n_sel), rank_tr_clamp(p0 + pl, a.n), a.n)];
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < RANKV_T * RANKV_T / RANKV_THREADS; ++r) {
    const int pl = rank_tr_row(r, t), gl = rank_tr_lane(t);
    if (p0 + pl < a.n && j0 + gl < a.n_sel) a.out[rank_tr_dst(p0 + pl, j0 + gl, a.ld_out)] = tile[gl][pl];
  }
}

}  // namespace spv
