// Rank sums of the OBSERVED counts (spVIPES.rank_genes_groups of the user API: the Wilcoxon / Mann-Whitney rank-sum test of every
// label against the rest): a segmented column sort with tie runs.  For a list of n cells with a segment code each and a slab of
// selected genes, per gene the sum over every segment's cells of TWICE the cell's average rank, and the tie term sum (t^3 - t).
//
// The arithmetic.  The key of list position p in gene j is ONE fp32 product, key = (float)count * w[p] (w == NULL: (float)count),
// never contracted with anything.  Keys are non-negative, so their bit pattern orders them.  With L = the number of list positions
// with a smaller key and U = the number with a smaller or equal key, L + U + 1 is twice the average rank of the position: an integer.
// Every output is an integer sum, so the order of addition is free: 64-bit INTEGER atomics (LDS) collect them, there is no
// floating-point atomic anywhere, and two calls agree bit for bit whatever order the hardware took.
//
// How the work is laid out on the chip
//   * stage (rank_stage_kernel): one workgroup per tile of RANK_TP list positions x RANK_TG selected genes.  Lanes run along genes
//     while the row pieces are read (the row gather; a row number and a weight are wave-uniform), the keys cross an LDS tile, and lanes
//     run along positions while they are written: a wave owns a gene, finds the tile's NON-ZERO keys of that gene with two ballots,
//     takes their places from the gene's cursor with ONE integer atomic and appends (key, segment) entries back to back, gene-major.
//     Single-cell counts are about 90 % zeros; all zero keys form one run at the bottom (L = 0, U = n_zero) and are never stored or
//     sorted.  The first gene tile's workgroups also count the list positions per segment (an LDS histogram, flushed with integer
//     atomics): a segment's zero keys are its positions minus its stored entries.
//   * sums (rank_sums_kernel): one workgroup of RANK_THREADS threads per gene sorts the gene's m stored entries and walks the tie runs.
//       m <= RANK_LDS_CAP : the column is loaded into LDS, padded to a power of two with all-ones entries, and sorted there by a
//                           bitonic network (compare-exchange in place: no scatter at all)
//       m >  RANK_LDS_CAP : least-significant-digit radix sort through global memory, 8-bit digits, ping-pong between the two halves of
//                           the workspace.  One pass over the column builds the four digit histograms; a pass whose digit is the same
//                           for every entry is skipped.  A pass moves the column in tiles of RANK_THREADS entries in order: every lane
//                           finds the lanes of its wave with the same digit (8 ballots), the first of them records the wave's count,
//                           256 threads turn the (wave, digit) counts into offsets behind the digit's running base, and every entry
//                           goes to base + earlier waves + earlier lanes -- stable, as an LSD sort needs.
//     The walk: entry i of the sorted column belongs to the run [s, e) of its key (a neighbour with another key ends the run at once,
//     else a binary search does); it adds 2 n_zero + s + e + 1 to its segment's sum, and the run's first entry adds t^3 - t, t = e - s.
//     A segment code outside [0, n_seg) is stored as n_seg: the entry is ranked with the others but adds to no sum.
//
// Every index bound
//   * stage, reads: a slot of the tile at or beyond p_end = pos_off + n_piece (<= n, the wrapper checks) reads position p_end - 1 instead
//     and is discarded; rows is read at q - pos_off in [0, n_piece), w at q and seg at p < p_end, both in [0, n).  A row number outside
//     [0, n_rows) and a gene outside [0, G) read as a zero count and are never dereferenced: the load goes to row 0 / gene 0 instead, which
//     exist (n_rows > 0, G > 0), and its value is dropped; the wrapper has checked ld >= col_off + G, so row * ld + col_off + gene is
//     inside the matrix for every row in [0, n_rows) and gene in [0, G).
//   * stage, writes: a gene's cursor grows by the number of non-zero keys appended, at most one per list position and gene, so a slot
//     is < n when every position is staged once.  A caller that stages a piece twice could push it beyond: a slot >= n is NOT written
//     (and rank_sums cuts m to n).  Entry address = gene slot j * n + slot < n_sel * n, inside half A of the workspace.
//   * sums, LDS path: indices of the network are < P = the power of two >= m, P <= RANK_LDS_CAP.
//   * sums, radix path: the histogram counts exactly the entries a pass moves, so digit base + earlier waves + earlier lanes < m; the
//     store is guarded by dst < m all the same.  Both halves hold n entries per gene, m <= n.
//   * sums, outputs: rank2[k * ld_rank2 + j], k < n_seg, j < n_sel <= ld_rank2; ties[j].  The segment accumulators are indexed by a
//     stored code, which is <= n_seg by construction and used only when < n_seg <= RANK_MAX_SEG.
#pragma once
#include "spv_common.h"

namespace spv {

// ---- RANK-CORE-BEGIN ----
// (plain C++: tools/rank_host_check.py compiles this text for the host and runs it behind an emulated workgroup)
constexpr int RANK_MAX_N = 1 << 20;     // list positions, at most
constexpr int RANK_MAX_SEG = 1024;      // segments, at most
constexpr int RANK_SLAB = 1024;         // selected genes per call, at most (one cursor each)
constexpr int RANK_TP = 128;            // stage tile: list positions
constexpr int RANK_TG = 64;             //             selected genes
constexpr int RANK_UNROLL = 8;          //             rows in flight per wave
constexpr int RANK_THREADS = 1024;      // threads of a sums workgroup = entries per radix tile
constexpr int RANK_WAVES = RANK_THREADS / 64;
constexpr int RANK_LDS_CAP = 8192;      // entries an LDS-resident sort holds (64 KiB)
constexpr long long RANK_WS_HEAD = (long long)(RANK_SLAB + RANK_MAX_SEG) * 4;   // cursor int32 [RANK_SLAB], segcnt int32 [RANK_MAX_SEG]

typedef unsigned long long rank_entry_t;   // key bits << 32 | segment code (n_seg: counted in no sum)

// workspace: [cursor][segcnt][half A: n_sel columns of n entries][half B: the same]; byte offsets
__host__ __device__ __forceinline__ long long rank_ws_cursor_off() { return 0; }
__host__ __device__ __forceinline__ long long rank_ws_segcnt_off() { return (long long)RANK_SLAB * 4; }
__host__ __device__ __forceinline__ long long rank_ws_half_off(int half, int n, int n_sel) { return RANK_WS_HEAD + (long long)half * n * n_sel * 8; }
__host__ __device__ __forceinline__ long long rank_ws_bytes(int n, int n_sel) {
  if (n <= 0 || n_sel <= 0 || n > RANK_MAX_N || n_sel > RANK_SLAB) return 0;
  return RANK_WS_HEAD + 2ll * n * n_sel * 8;
}

// the key image: ONE fp32 multiply (fp contraction off), its bit pattern; any zero key is the pattern 0
__host__ __device__ __forceinline__ unsigned rank_key_bits(float c, float w, bool has_w) {
#pragma clang fp contract(off)
  const float k = has_w ? c * w : c;
  return k != 0.f ? __builtin_bit_cast(unsigned, k) : 0u;
}
__host__ __device__ __forceinline__ rank_entry_t rank_entry(unsigned key, int code, int n_seg) {
  return ((rank_entry_t)key << 32) | (unsigned)(code >= 0 && code < n_seg ? code : n_seg);
}
// the rank transform's entry (spv_rank_values.h): the low word is the LIST POSITION itself (read back with rank_entry_seg)
__host__ __device__ __forceinline__ rank_entry_t rank_pos_entry(unsigned key, int p) { return ((rank_entry_t)key << 32) | (unsigned)p; }
__host__ __device__ __forceinline__ unsigned rank_entry_key(rank_entry_t e) { return (unsigned)(e >> 32); }
__host__ __device__ __forceinline__ unsigned rank_entry_seg(rank_entry_t e) { return (unsigned)e; }

// stage reads: the list position whose row number and weight a slot of the tile reads (a position of the piece that exists, whatever the
// slot: n_piece > 0), and the element a lane loads -- the cell's own when it counts, else row 0's (n_rows > 0, ld >= col_off + G > col_off + gene)
__host__ __device__ __forceinline__ int rank_stage_position(int p, int p_end) { return p < p_end ? p : p_end - 1; }
__host__ __device__ __forceinline__ long rank_stage_source(bool counts, int row, long ld, int col_off, int gene) {
  return (long)(counts ? row : 0) * ld + col_off + gene;
}

// the smallest power of two >= m (>= 1)
__host__ __device__ __forceinline__ int rank_pow2(int m) {
  int p = 1;
  while (p < m) p <<= 1;
  return p;
}
// compare-exchange t of step (k, j) of the bitonic network over a[0 .. P): the pair (i, i | j), ascending where (i & k) == 0
__host__ __device__ __forceinline__ void rank_bitonic_cx(rank_entry_t* a, int t, int j, int k) {
  const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
  const rank_entry_t x = a[i], y = a[l];
  if ((x > y) == ((i & k) == 0)) { a[i] = y; a[l] = x; }
}

// radix: the digit of pass `pass` (8 bits, least significant first), and the lanes of a wave that hold the same digit, from the
// ballots of the digit's 8 bits (bal[b]: the lanes whose bit b is set) among the `valid` lanes
__host__ __device__ __forceinline__ unsigned rank_digit(unsigned key, int pass) { return (key >> (8 * pass)) & 255u; }
__host__ __device__ __forceinline__ unsigned long long rank_peers(const unsigned long long* bal, unsigned digit, unsigned long long valid) {
  unsigned long long p = valid;
  for (int b = 0; b < 8; ++b) p &= ((digit >> b) & 1u) ? bal[b] : ~bal[b];
  return p;
}
__host__ __device__ __forceinline__ int rank_popc(unsigned long long v) { return __builtin_popcountll(v); }
__host__ __device__ __forceinline__ unsigned long long rank_lanes_below(int lane) { return (1ull << lane) - 1ull; }

// the run [s, e) of entry i's key in a sorted column of m entries
__host__ __device__ __forceinline__ int rank_run_begin(const rank_entry_t* a, int i) {
  const unsigned key = rank_entry_key(a[i]);
  if (i == 0 || rank_entry_key(a[i - 1]) != key) return i;
  int lo = 0, hi = i - 1;   // the first index in [0, i - 1] whose key is not smaller (a[i - 1] has it)
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (rank_entry_key(a[mid]) < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}
__host__ __device__ __forceinline__ int rank_run_end(const rank_entry_t* a, int i, int m) {
  const unsigned key = rank_entry_key(a[i]);
  if (i + 1 == m || rank_entry_key(a[i + 1]) != key) return i + 1;
  int lo = i + 2, hi = m;   // the first index in [i + 2, m] whose key is larger (m: none)
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (rank_entry_key(a[mid]) > key) hi = mid; else lo = mid + 1;
  }
  return lo;
}
// L + U + 1 of an entry of the run [s, e) above n_zero zero keys; t^3 - t of a run of t; what a segment's zero keys add
__host__ __device__ __forceinline__ unsigned long long rank_elem_term(int n_zero, int s, int e) { return 2ull * n_zero + s + e + 1ull; }
__host__ __device__ __forceinline__ unsigned long long rank_tie_term(int t) { return (unsigned long long)t * t * t - t; }
__host__ __device__ __forceinline__ unsigned long long rank_zero_term(int seg_positions, int seg_stored, int n_zero) {
  return (unsigned long long)(seg_positions - seg_stored) * (n_zero + 1ull);   // L = 0, U = n_zero for each of them
}
// ---- RANK-CORE-END ----

struct RankArgs {
  const void* X; long ld; const int* rows; int col_off;   // the matrix; list position p -> rows[p - pos_off] (nullptr: p - pos_off)
  int G, n_rows, n_piece, pos_off;                        // positions [pos_off, pos_off + n_piece) are addressable through this matrix
  int n, n_seg, n_sel;
  const int* seg; const float* w; const int* genes;
  long long* rank2; long ld_rank2; long long* ties;
  char* ws;
};

// the first piece of a list starts from empty columns: the cursors and the segment counts are zeroed (an ordinary launch)
__global__ __launch_bounds__(256) void rank_reset_kernel(int* head) {
  head[blockIdx.x * 256 + threadIdx.x] = 0;   // (the grid covers exactly RANK_SLAB + RANK_MAX_SEG words, a multiple of 256)
}

// POS (the rank transform, spv_rank_values.h): an entry's low word is the list position p, not a segment code -- seg is not read, no
// histogram is built or flushed (count_segments is a constant false and the code behind it is dropped).  POS == false is the kernel above.
template <bool U16, bool POS>
__global__ __launch_bounds__(256) void rank_stage_kernel(RankArgs a) {
  __shared__ unsigned tile[RANK_TG][RANK_TP + 1];   // (+ 1: a wave writes one position of 64 genes, 129 words apart -> 64 banks)
  __shared__ int hist[POS ? 1 : RANK_MAX_SEG];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int p0 = a.pos_off + (int)blockIdx.x * RANK_TP, p_end = a.pos_off + a.n_piece, j0 = (int)blockIdx.y * RANK_TG;
  const bool count_segments = !POS && blockIdx.y == 0;
  if (count_segments) {
    for (int k = threadIdx.x; k < RANK_MAX_SEG; k += 256) hist[k] = 0;
  }
  // read: lanes along genes, the waves take the tile's positions round-robin
  const int j = j0 + lane;
  int g = -1;
  if (j < a.n_sel) g = a.genes ? a.genes[j] : j;
  const bool g_ok = g >= 0 && g < a.G;
  // RANK_UNROLL positions per round: every load is issued UNCONDITIONALLY from an address that exists (rank_stage_source) and what does not
  // belong is discarded afterwards, so that a round's loads go out back to back and are waited for once (a load inside a branch is waited
  // for at the branch's end: the first build did that and read the matrix at 139 GB/s)
  for (int pl0 = wave; pl0 < RANK_TP; pl0 += 4 * RANK_UNROLL) {
    float c[RANK_UNROLL], wv[RANK_UNROLL];
    bool ok[RANK_UNROLL];
#pragma unroll
    for (int u = 0; u < RANK_UNROLL; ++u) {
      const int q = rank_stage_position(p0 + pl0 + 4 * u, p_end);
      const int r = a.rows ? a.rows[q - a.pos_off] : q - a.pos_off;
      ok[u] = p0 + pl0 + 4 * u < p_end && r >= 0 && r < a.n_rows && g_ok;
      const long at = rank_stage_source(ok[u], r, a.ld, a.col_off, g_ok ? g : 0);
      if constexpr (U16) c[u] = (float)reinterpret_cast<const unsigned short*>(a.X)[at];
      else c[u] = reinterpret_cast<const float*>(a.X)[at];
      wv[u] = a.w ? a.w[q] : 1.f;
    }
#pragma unroll
    for (int u = 0; u < RANK_UNROLL; ++u) tile[lane][pl0 + 4 * u] = ok[u] ? rank_key_bits(c[u], wv[u], a.w != nullptr) : 0u;
  }
  // the segment codes of this lane's two positions (lanes along positions from here on)
  int code[2];
  bool live[2];
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int p = p0 + 64 * c + lane;
    live[c] = p < p_end;
    if constexpr (POS) code[c] = p;
    else code[c] = live[c] ? a.seg[p] : -1;
  }
  __syncthreads();
  if (count_segments && wave == 0) {
#pragma unroll
    for (int c = 0; c < 2; ++c)
      if (live[c] && code[c] >= 0 && code[c] < a.n_seg) atomicAdd(&hist[code[c]], 1);
  }
  // append: a wave owns a gene of the tile at a time
  int* const cursor = reinterpret_cast<int*>(a.ws + rank_ws_cursor_off());
  rank_entry_t* const half_a = reinterpret_cast<rank_entry_t*>(a.ws + rank_ws_half_off(0, a.n, a.n_sel));
  const unsigned long long below = rank_lanes_below(lane);
  for (int gl = wave; gl < RANK_TG; gl += 4) {
    const int jj = j0 + gl;
    if (jj >= a.n_sel) break;   // (wave-uniform)
    const unsigned k0 = tile[gl][lane], k1 = tile[gl][64 + lane];
    const unsigned long long b0 = __ballot(k0 != 0u), b1 = __ballot(k1 != 0u);
    const int c0 = rank_popc(b0), cnt = c0 + rank_popc(b1);
    if (cnt == 0) continue;
    int base = 0;
    if (lane == 0) base = atomicAdd(&cursor[jj], cnt);
    base = __shfl(base, 0, 64);
    rank_entry_t* const col = half_a + (long)jj * a.n;
    if (k0 != 0u) {
      const int slot = base + rank_popc(b0 & below);
      if (slot >= 0 && slot < a.n) col[slot] = POS ? rank_pos_entry(k0, code[0]) : rank_entry(k0, code[0], a.n_seg);
    }
    if (k1 != 0u) {
      const int slot = base + c0 + rank_popc(b1 & below);
      if (slot >= 0 && slot < a.n) col[slot] = POS ? rank_pos_entry(k1, code[1]) : rank_entry(k1, code[1], a.n_seg);
    }
  }
  if (count_segments) {
    __syncthreads();
    int* const segcnt = reinterpret_cast<int*>(a.ws + rank_ws_segcnt_off());
    for (int k = threadIdx.x; k < a.n_seg; k += 256)
      if (hist[k]) atomicAdd(&segcnt[k], hist[k]);
  }
}

struct RankRadixLds {   // the radix path's view of the sort buffer
  unsigned hist[4][256];
  unsigned wavecnt[RANK_WAVES][256];
  unsigned run[4][256];   // per pass: the digit's running base
  unsigned wtot[RANK_WAVES];
  int skip[4];            // per pass: every entry has the same digit (written once, before the passes)
};
static_assert(sizeof(RankRadixLds) <= sizeof(rank_entry_t) * RANK_LDS_CAP, "the radix tables live in the LDS sort buffer");

// The sort both walks share (rank_sums_kernel here, rank_values_kernel of spv_rank_values.h): the whole workgroup of RANK_THREADS
// threads sorts the m (<= n) entries of one column ascending -- in buf (LDS, RANK_LDS_CAP entries) up to RANK_LDS_CAP, else by the
// radix passes between src and dst (n entries each) with buf as their tables -- and returns where the sorted column stands; a barrier
// has made it visible to every thread.  Every thread must call it with the same arguments.
__device__ __forceinline__ const rank_entry_t* rank_sort_column(rank_entry_t* buf, rank_entry_t* src, rank_entry_t* dst, const int m) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const rank_entry_t* sorted;
  if (m <= RANK_LDS_CAP) {
    const int P = rank_pow2(m);
    for (int i = tid; i < P; i += RANK_THREADS) buf[i] = i < m ? src[i] : ~0ull;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
      for (int jj = k >> 1; jj > 0; jj >>= 1) {
        for (int t = tid; t < (P >> 1); t += RANK_THREADS) rank_bitonic_cx(buf, t, jj, k);
        __syncthreads();
      }
    sorted = buf;
  } else {
    RankRadixLds& R = *reinterpret_cast<RankRadixLds*>(buf);
    for (int i = tid; i < 4 * 256; i += RANK_THREADS) (&R.hist[0][0])[i] = 0u;
    if (tid < 4) R.skip[tid] = 0;
    __syncthreads();
    for (int i = tid; i < m; i += RANK_THREADS) {
      const unsigned key = rank_entry_key(src[i]);
#pragma unroll
      for (int ps = 0; ps < 4; ++ps) atomicAdd(&R.hist[ps][rank_digit(key, ps)], 1u);
    }
    __syncthreads();
    // all four passes are prepared at once, four waves per pass and a thread per digit: the digit bases (an exclusive scan of the pass's
    // histogram: inside the wave by shuffles, across the pass's four waves through wtot) and whether the pass is skipped.  R.skip is
    // written here only and read once into a register behind the barrier, so every thread of the workgroup takes the same passes.
    {
      const int ps = tid >> 8, d = tid & 255;
      const unsigned v = R.hist[ps][d];
      if (v == (unsigned)m) R.skip[ps] = 1;   // every entry has this digit (m > 0: at most one digit of a pass): the pass would move nothing
      unsigned inc = v;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const unsigned t = __shfl_up(inc, off, 64);
        if (lane >= off) inc += t;
      }
      if (lane == 63) R.wtot[wave] = inc;
      __syncthreads();
      unsigned base = 0u;
      for (int w = wave & ~3; w < wave; ++w) base += R.wtot[w];
      R.run[ps][d] = base + inc - v;
    }
    int skip = 0;
#pragma unroll
    for (int ps = 0; ps < 4; ++ps) skip |= R.skip[ps] ? 1 << ps : 0;
    __syncthreads();
    const unsigned long long below = rank_lanes_below(lane);
    for (int ps = 0; ps < 4; ++ps) {
      if ((skip >> ps) & 1) continue;   // (a register filled from LDS words that no one writes after the barrier above: uniform over the workgroup)
      for (int t0 = 0; t0 < m; t0 += RANK_THREADS) {
        const int i = t0 + tid;
        const bool valid = i < m;
        const rank_entry_t e = valid ? src[i] : 0ull;
        const unsigned d = rank_digit(rank_entry_key(e), ps);
        unsigned long long bal[8];
#pragma unroll
        for (int b = 0; b < 8; ++b) bal[b] = __ballot((d >> b) & 1u);
        const unsigned long long peers = rank_peers(bal, d, __ballot(valid));
        const int before = rank_popc(peers & below);
#pragma unroll
        for (int q = 0; q < 4; ++q) R.wavecnt[wave][lane + 64 * q] = 0u;
        __builtin_amdgcn_wave_barrier();
        if (valid && before == 0) R.wavecnt[wave][d] = (unsigned)rank_popc(peers);
        __syncthreads();
        if (tid < 256) {   // (wave, digit) counts -> offsets behind the digit's running base
          unsigned s = R.run[ps][tid];
          for (int w = 0; w < RANK_WAVES; ++w) {
            const unsigned c = R.wavecnt[w][tid];
            R.wavecnt[w][tid] = s;
            s += c;
          }
          R.run[ps][tid] = s;
        }
        __syncthreads();
        if (valid) {
          const unsigned at = R.wavecnt[wave][d] + (unsigned)before;
          if (at < (unsigned)m) dst[at] = e;
        }
        __syncthreads();
      }
      rank_entry_t* const t = src; src = dst; dst = t;   // (the barrier above has made the stores visible to the workgroup)
    }
    sorted = src;
  }
  __syncthreads();
  return sorted;
}

__global__ __launch_bounds__(RANK_THREADS) void rank_sums_kernel(RankArgs a) {
  __shared__ rank_entry_t buf[RANK_LDS_CAP];
  __shared__ unsigned long long acc[RANK_MAX_SEG];
  __shared__ int stored[RANK_MAX_SEG];
  __shared__ unsigned long long tie;
  const int tid = threadIdx.x, j = blockIdx.x;
  const int* const cursor = reinterpret_cast<const int*>(a.ws + rank_ws_cursor_off());
  const int* const segcnt = reinterpret_cast<const int*>(a.ws + rank_ws_segcnt_off());
  const int m = min(max(cursor[j], 0), a.n), n_zero = a.n - m;
  rank_entry_t* src = reinterpret_cast<rank_entry_t*>(a.ws + rank_ws_half_off(0, a.n, a.n_sel)) + (long)j * a.n;
  rank_entry_t* dst = reinterpret_cast<rank_entry_t*>(a.ws + rank_ws_half_off(1, a.n, a.n_sel)) + (long)j * a.n;
  for (int k = tid; k < a.n_seg; k += RANK_THREADS) { acc[k] = 0ull; stored[k] = 0; }
  if (tid == 0) tie = 0ull;
  const rank_entry_t* const sorted = rank_sort_column(buf, src, dst, m);
  for (int i = tid; i < m; i += RANK_THREADS) {
    const int s = rank_run_begin(sorted, i), e = rank_run_end(sorted, i, m);
    const unsigned sg = rank_entry_seg(sorted[i]);
    if (sg < (unsigned)a.n_seg) {
      atomicAdd(&acc[sg], rank_elem_term(n_zero, s, e));
      atomicAdd(&stored[sg], 1);
    }
    if (s == i) atomicAdd(&tie, rank_tie_term(e - s));
  }
  __syncthreads();
  for (int k = tid; k < a.n_seg; k += RANK_THREADS)
    a.rank2[(long)k * a.ld_rank2 + j] = (long long)(acc[k] + rank_zero_term(segcnt[k], stored[k], n_zero));
  if (tid == 0) a.ties[j] = (long long)(tie + rank_tie_term(n_zero));
}

}  // namespace spv
