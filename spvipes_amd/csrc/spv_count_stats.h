// Statistics of the OBSERVED counts per population (spVIPES.count_statistics of the user API): per segment (label) and gene the sum
// of the counts, the number of listed cells with a non-zero count and the weighted sum, over listed rows of a resident count matrix
// (spv_count_stats), and the per-cell totals the weights are made from (spv_count_totals, spv_csr_totals).
//
// How the work is laid out on the chip
//   * The list of cells is cut into slabs of at most CS_SLAB list positions, none of which crosses a segment (the host builds the
//     table).  The partial pass runs one workgroup per (slab, gene tile of CS_TILE genes): lanes run along genes, 8 consecutive
//     genes per lane as one 16-byte load of uint16 counts (two 16-byte loads of 4 fp32 counts each), so a wave reads 1 KiB (2 KiB)
//     of a row per step; the CS_WAVES waves of the workgroup take the slab's cells round-robin.  A cell's row number and weight are
//     wave-uniform (scalar loads), fetched for CS_UNROLL cells before the first of their rows is used, and the CS_UNROLL row pieces
//     are all issued before the first is summed: the row gathers are the whole cost.
//   * The vector loads need (row * ld + col_off) to fall on a 16-byte boundary for EVERY row: the wrapper checks the base pointer,
//     ld and col_off once and launches the element-wise instantiation (VEC = false) of the same kernel otherwise (also when G is
//     smaller than one 16-byte piece).  In the vector
//     instantiation the one lane that straddles gene G reads its genes one by one.
//   * Reduction, in a fixed order throughout (no floating-point atomics; two calls agree bit for bit):
//       lane      : uint16 counts add into 32-bit integer sums (a lane sees at most CS_SLAB cells: CS_SLAB * 65535 < 2^31), fp32
//                   counts are widened (exact) and added in fp64; the non-zero tally is an integer; the weighted term is ONE fp64
//                   multiply (fp contraction is off in cs_add: no fused multiply-add), added in fp64 in list order
//       workgroup : waves 1 .. CS_WAVES-1 hand their sums to wave 0 through LDS, which adds them in wave order in fp64 and writes
//                   one record per (slab, gene) to the workspace ws[slab][3][G]
//       merge     : one thread per selected gene adds its segment's slab records in slab order -> out[segment][3][ld_out]
//     The partial pass always covers all G genes, so a selected column equals the same column of an all-genes call bit for bit.
#pragma once
#include "spv_common.h"

namespace spv {

constexpr int CS_TILE = 512;     // genes per workgroup of the partial pass: 64 lanes x 8
constexpr int CS_SLAB = 512;     // list positions per slab, at most (the host's plan; any value <= CS_SLAB_MAX is accepted)
constexpr int CS_SLAB_MAX = 32768;   // 32768 * 65535 < 2^31: a lane's integer sums cannot overflow
constexpr int CS_WAVES = 4;      // waves per workgroup of the partial pass
constexpr int CS_UNROLL = 4;     // rows in flight per wave

struct CsArgs {
  const void* X; long ld; const int* rows; int col_off;   // the matrix; rows: list position p -> rows[p - pos_off] (nullptr: p - pos_off)
  int G, n_rows, n, pos_off;                               // n list positions [pos_off, pos_off + n) are addressable through this matrix
  const double* w;                                         // [.] indexed by LIST POSITION (nullptr: 1)
  const int* genes; int n_sel;
  const int* slabs;                                        // [n_slabs][3]: begin, end (list positions), segment
  const int* seg_slabs;                                    // [n_seg + 1]: segment k owns slabs [seg_slabs[k], seg_slabs[k + 1])
  int n_slabs, n_seg, slab_first, slab_count;              // the partial pass runs slabs [slab_first, slab_first + slab_count)
  double* out; long ld_out;
  double* ws;                                              // [n_slabs][3][G]
};

// the gene of a lane's i-th value, relative to the tile: uint16 8 consecutive genes; fp32 two runs of 4, 256 genes apart
template <bool U16>
__device__ __forceinline__ int cs_gene(int lane, int i) {
  if constexpr (U16) return lane * 8 + i;
  else return (i >> 2) * 256 + lane * 4 + (i & 3);
}

template <bool U16> struct CsRow;
template <> struct CsRow<true> { u4v q; };
template <> struct CsRow<false> { f4v a, b; };

// One row piece of this lane, 8 counts, comes in one of two ways.  Both issue their loads UNCONDITIONALLY from an address that
// exists and discard what does not belong (the address is selected, not the load skipped), so that the loads of CS_UNROLL rows go out
// back to back and are waited for once.  `off`: the element offset of the row's first gene -- row 0's when the row does not exist
// (cs_fetch), so a row number outside the matrix is never dereferenced.
//   cs_issue_vec  : 16-byte loads; a lane whose genes do not all lie below G reads row 0's first piece instead (the wrapper has checked
//                   that every row is 16-byte aligned and that G holds one whole piece)
//   cs_issue_elems: 8 element loads, a gene at or beyond G reads gene G - 1 instead
// cs_take_* then zero what was not asked for: a row that does not exist (`ok`, wave-uniform) and genes at or beyond G.
template <bool U16>
__device__ __forceinline__ CsRow<U16> cs_issue_vec(const void* X, int col_off, long off, int t0, int lane, int G) {
  CsRow<U16> r;
  if constexpr (U16) {
    const unsigned short* const x = reinterpret_cast<const unsigned short*>(X);
    const int g0 = t0 + lane * 8;
    r.q = *reinterpret_cast<const u4v*>(g0 + 8 <= G ? x + off + g0 : x + col_off);
  } else {
    const float* const x = reinterpret_cast<const float*>(X);
    const int ga = t0 + lane * 4, gb = ga + 256;
    r.a = *reinterpret_cast<const f4v*>(ga + 4 <= G ? x + off + ga : x + col_off);
    r.b = *reinterpret_cast<const f4v*>(gb + 4 <= G ? x + off + gb : x + col_off);
  }
  return r;
}
template <bool U16>
__device__ __forceinline__ CsRow<U16> cs_take_vec(CsRow<U16> r, bool ok, int t0, int lane, int G) {
  if constexpr (U16) {
    if (!(ok && t0 + lane * 8 + 8 <= G)) r.q = u4v{0u, 0u, 0u, 0u};
  } else {
    const int ga = t0 + lane * 4, gb = ga + 256;
    if (!(ok && ga + 4 <= G)) r.a = f4v{0.f, 0.f, 0.f, 0.f};
    if (!(ok && gb + 4 <= G)) r.b = f4v{0.f, 0.f, 0.f, 0.f};
  }
  return r;
}

template <bool U16> struct CsElems;
template <> struct CsElems<true> { unsigned short v[8]; };
template <> struct CsElems<false> { float v[8]; };

template <bool U16>
__device__ __forceinline__ CsElems<U16> cs_issue_elems(const void* X, long off, int t0, int lane, int G) {
  CsElems<U16> r;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int g = min(t0 + cs_gene<U16>(lane, i), G - 1);
    if constexpr (U16) r.v[i] = reinterpret_cast<const unsigned short*>(X)[off + g];
    else r.v[i] = reinterpret_cast<const float*>(X)[off + g];
  }
  return r;
}
template <bool U16>
__device__ __forceinline__ CsRow<U16> cs_take_elems(const CsElems<U16>& r, bool ok, int t0, int lane, int G) {
  CsRow<U16> o;
  if constexpr (U16) {
    o.q = u4v{0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < 8; ++i)
      o.q[i >> 1] |= (ok && t0 + cs_gene<true>(lane, i) < G ? (unsigned)r.v[i] : 0u) << (16 * (i & 1));
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float v = ok && t0 + cs_gene<false>(lane, i) < G ? r.v[i] : 0.f;
      if (i < 4) o.a[i & 3] = v;
      else o.b[i & 3] = v;
    }
  }
  return o;
}

template <bool U16> struct CsLane;
template <> struct CsLane<true> { unsigned s[8]; unsigned nz[8]; double ws[8]; };
template <> struct CsLane<false> { double s[8]; unsigned nz[8]; double ws[8]; };

// fold one row piece into the lane's sums: sum, non-zero tally, and fl64(count * w) added in fp64 (a multiply and an add, never fused)
template <bool U16>
__device__ __forceinline__ void cs_add(CsLane<U16>& l, const CsRow<U16>& r, double w) {
#pragma clang fp contract(off)
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    if constexpr (U16) {
      const unsigned v = (i & 1) ? (r.q[i >> 1] >> 16) : (r.q[i >> 1] & 0xFFFFu);
      l.s[i] += v;
      l.nz[i] += v != 0u ? 1u : 0u;
      const double t = (double)v * w;
      l.ws[i] = l.ws[i] + t;
    } else {
      const float v = i < 4 ? r.a[i & 3] : r.b[i & 3];
      const double d = (double)v;
      l.s[i] = l.s[i] + d;
      l.nz[i] += v != 0.f ? 1u : 0u;
      const double t = d * w;
      l.ws[i] = l.ws[i] + t;
    }
  }
}

struct CsIdx { long off[CS_UNROLL]; bool ok[CS_UNROLL]; double w[CS_UNROLL]; };

// list positions p, p + CS_WAVES, ... of a slab that ends at e: element offset of the row's first gene, whether the row exists, its weight.
// A position at or beyond e, and a row number outside [0, n_rows), give ok = false: nothing is read through them.
__device__ __forceinline__ void cs_fetch(CsIdx& x, const CsArgs& a, int p, int e) {
#pragma unroll
  for (int u = 0; u < CS_UNROLL; ++u) {
    const int pp = p + u * CS_WAVES;
    const bool in = pp < e;
    const int q = in ? pp : a.pos_off;   // (a position that exists, whatever `in` says: n > 0)
    const int r = a.rows ? a.rows[q - a.pos_off] : q - a.pos_off;
    x.ok[u] = in && r >= 0 && r < a.n_rows;
    x.off[u] = (long)(x.ok[u] ? r : 0) * a.ld + a.col_off;
    x.w[u] = a.w ? a.w[q] : 1.0;
  }
}

template <bool U16, bool VEC>
__global__ __launch_bounds__(64 * CS_WAVES) void count_stats_partial_kernel(CsArgs a) {
  __shared__ double sm[CS_WAVES - 1][24][64];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int tiles = (a.G + CS_TILE - 1) / CS_TILE;
  const int slab = a.slab_first + (int)(blockIdx.x / tiles), t0 = (int)(blockIdx.x % tiles) * CS_TILE;
  // the slab's list positions, cut to what this call can address (a table that says otherwise reads nothing outside it)
  int b = a.slabs[3 * slab], e = a.slabs[3 * slab + 1];
  b = max(b, a.pos_off);
  e = min(e, a.pos_off + a.n);
  if (e - b > CS_SLAB_MAX) e = b + CS_SLAB_MAX;
  CsLane<U16> l;
#pragma unroll
  for (int i = 0; i < 8; ++i) { l.s[i] = 0; l.nz[i] = 0u; l.ws[i] = 0.0; }
  // the row numbers and weights of CS_UNROLL cells (p, u are wave-uniform: scalar loads and scalar compares); they are fetched one
  // round ahead of the rows they address, right after the current round's row loads have been issued
  // a lane of the vector instantiation whose piece straddles gene G (fp32: either of its two runs) reads its genes one by one
  const int run = U16 ? 8 : 4, g_first = t0 + cs_gene<U16>(lane, 0), g_second = t0 + cs_gene<U16>(lane, 4);
  const bool part = (g_first < a.G && g_first + run > a.G) || (!U16 && g_second < a.G && g_second + run > a.G);
  CsIdx cur, nxt;
  cs_fetch(cur, a, b + wave, e);
  for (int p = b + wave; p < e; p += CS_WAVES * CS_UNROLL) {
    if constexpr (VEC) {
      CsRow<U16> row[CS_UNROLL];
#pragma unroll
      for (int u = 0; u < CS_UNROLL; ++u) row[u] = cs_issue_vec<U16>(a.X, a.col_off, cur.off[u], t0, lane, a.G);
      cs_fetch(nxt, a, p + CS_WAVES * CS_UNROLL, e);
#pragma unroll
      for (int u = 0; u < CS_UNROLL; ++u) {
        CsRow<U16> r = cs_take_vec<U16>(row[u], cur.ok[u], t0, lane, a.G);
        if (part) r = cs_take_elems<U16>(cs_issue_elems<U16>(a.X, cur.off[u], t0, lane, a.G), cur.ok[u], t0, lane, a.G);   // (one lane of the last tile)
        cs_add<U16>(l, r, cur.w[u]);   // (a row that does not exist is all zeros: it adds nothing)
      }
    } else {
      CsElems<U16> row[CS_UNROLL];
#pragma unroll
      for (int u = 0; u < CS_UNROLL; ++u) row[u] = cs_issue_elems<U16>(a.X, cur.off[u], t0, lane, a.G);
      cs_fetch(nxt, a, p + CS_WAVES * CS_UNROLL, e);
#pragma unroll
      for (int u = 0; u < CS_UNROLL; ++u) cs_add<U16>(l, cs_take_elems<U16>(row[u], cur.ok[u], t0, lane, a.G), cur.w[u]);
    }
    cur = nxt;
  }
  // waves 1.. hand their sums to wave 0, which adds them in wave order
  if (wave > 0) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      sm[wave - 1][i][lane] = (double)l.s[i];
      sm[wave - 1][8 + i][lane] = (double)l.nz[i];
      sm[wave - 1][16 + i][lane] = l.ws[i];
    }
  }
  __syncthreads();
  if (wave == 0) {
    double* const o = a.ws + (long)slab * 3 * a.G;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      double s = (double)l.s[i], nz = (double)l.nz[i], ws = l.ws[i];
      for (int v = 0; v < CS_WAVES - 1; ++v) {
        s += sm[v][i][lane]; nz += sm[v][8 + i][lane]; ws += sm[v][16 + i][lane];
      }
      const int g = t0 + cs_gene<U16>(lane, i);
      if (g < a.G) { o[g] = s; o[(long)a.G + g] = nz; o[2 * (long)a.G + g] = ws; }
    }
  }
}

// out[k][f][j] = the sum over segment k's slabs, in slab order, of ws[slab][f][genes[j]]
__global__ __launch_bounds__(256) void count_stats_merge_kernel(CsArgs a) {
  const int j = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y;
  if (j >= a.n_sel) return;
  const int g = a.genes ? a.genes[j] : j;
  double s = 0.0, nz = 0.0, ws = 0.0;
  if (g >= 0 && g < a.G) {
    const int s0 = max(a.seg_slabs[k], 0), s1 = min(a.seg_slabs[k + 1], a.n_slabs);
    for (int sl = s0; sl < s1; ++sl) {
      const double* const i = a.ws + (long)sl * 3 * a.G + g;
      s += i[0]; nz += i[a.G]; ws += i[2 * (long)a.G];
    }
  }
  double* const o = a.out + (long)k * 3 * a.ld_out + j;
  o[0] = s; o[a.ld_out] = nz; o[2 * a.ld_out] = ws;
}

// ---- per-cell totals ---------------------------------------------------------------------------------------------------------
// One order for the dense and the CSR form, so that the two agree bit for bit: lane t of the cell's wave adds the counts of the
// genes g = t (mod 64) in ascending g, and the 64 lane sums are folded by halves (lane t += lane t + 32, then + 16, ... + 1).
// uint16 counts add as 64-bit integers (exact whatever the order); fp32 counts are widened and added in fp64.  A gene without a
// stored entry adds an exact zero, which changes no fp64 sum of non-negative terms.
__device__ __forceinline__ double cs_fold(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}
__device__ __forceinline__ unsigned long long cs_fold(unsigned long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

template <bool U16>
__global__ __launch_bounds__(256) void count_totals_kernel(const void* X, long ld, int col_off, int n_cells, int G, double* total) {
  const int lane = threadIdx.x & 63, c = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= n_cells) return;   // (whole waves leave: c is wave-uniform)
  if constexpr (U16) {
    const unsigned short* const p = reinterpret_cast<const unsigned short*>(X) + (long)c * ld + col_off;
    unsigned long long s = 0;
    for (int g = lane; g < G; g += 64) s += p[g];
    s = cs_fold(s);
    if (lane == 0) total[c] = (double)s;
  } else {
    const float* const p = reinterpret_cast<const float*>(X) + (long)c * ld + col_off;
    double s = 0.0;
    for (int g = lane; g < G; g += 64) s += (double)p[g];
    s = cs_fold(s);
    if (lane == 0) total[c] = s;
  }
}

// CSR: one wave per row over vals[indptr[r] .. indptr[r + 1]).  uint16: lanes stride over the entries.  fp32: the entries are taken
// 64 at a time in storage order (ascending gene); an entry of gene g belongs to lane g mod 64's sum, which lives in LDS; entries of
// one step that meet in a sum are added lowest lane (lowest gene) first, found with an integer LDS minimum.
template <bool U16>
__global__ __launch_bounds__(256) void csr_totals_kernel(const long* indptr, const int* cols, const void* vals, int n_cells, int G, double* total) {
  __shared__ double acc[4][64];
  __shared__ unsigned owner[4][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, c = blockIdx.x * 4 + wv;
  if (c >= n_cells) return;   // (no workgroup barrier below: the waves are independent)
  const long i0 = indptr[c], i1 = indptr[c + 1];
  if constexpr (U16) {
    const unsigned short* const v = reinterpret_cast<const unsigned short*>(vals);
    unsigned long long s = 0;
    for (long i = i0 + lane; i < i1; i += 64) s += v[i];
    s = cs_fold(s);
    if (lane == 0) total[c] = (double)s;
  } else {
    const float* const v = reinterpret_cast<const float*>(vals);
    acc[wv][lane] = 0.0;
    owner[wv][lane] = 64u;
    for (long base = i0; base < i1; base += 64) {   // (wave-uniform trip count)
      const long i = base + lane;
      bool todo = i < i1;
      const int g = todo ? cols[i] : 0;
      const double x = todo ? (double)v[i] : 0.0;
      todo = todo && g >= 0 && g < G;
      const int t = g & 63;
      while (__any(todo)) {
        if (todo) atomicMin(&owner[wv][t], (unsigned)lane);
        __builtin_amdgcn_wave_barrier();
        if (todo && owner[wv][t] == (unsigned)lane) { acc[wv][t] += x; todo = false; }
        __builtin_amdgcn_wave_barrier();
        owner[wv][lane] = 64u;
        __builtin_amdgcn_wave_barrier();
      }
    }
    const double s = cs_fold(acc[wv][lane]);
    if (lane == 0) total[c] = s;
  }
}

}  // namespace spv
