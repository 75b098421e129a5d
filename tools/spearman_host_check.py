#!/usr/bin/env python3
"""The rank transform's core on the CPU: compiles the text between the RANK-CORE marks of csrc/spv_rank.h and between the
RANK-VALUES-CORE marks of csrc/spv_rank_values.h -- the key image, the position entry, the stage's read maps, the bitonic
compare-exchange map, the tie-run walk, the value terms, the store's tile maps and the workspace layout and size, exactly as the kernels
use them -- as plain C++, with a driver that walks the grids the way rank_stage_kernel<., true>, rank_values_kernel and
rank_values_store_kernel do: the stage's tile with its ballots taken over the lanes and the gene cursors, in TWO pieces whenever the list
has two positions; per gene the fill of the fp32 column with the zero run's value, the sort (the bitonic network step by step up to the
LDS capacity; beyond it a plain stable sort by key stands in for the radix passes, which tools/rank_host_check.py walks), the scatter of
the stored entries' values by position; then the store, tile by tile through a [64][65] buffer with clamped reads and guarded writes.
Whole arrays are compared with numpy for EQUALITY:

  * the block must equal 2 * midrank - (n + 1) of the numpy float32 keys, ties the sum of t^3 - t, nonzero the stored keys per gene;
  * columns >= n_sel of the block must keep their sentinel;
  * the position word of every entry must be its list position (one shape lists more than 65 535 positions);
  * spv_rank_values_ws_bytes is spv_rank_ws_bytes + 4 n n_sel rounded up to 8, and 0 outside the ranges.
No GPU, nothing loaded into Python.  It checks everything except the hardware's atomics, ballots and barriers themselves.

    python tools/spearman_host_check.py [--sanitize] [--cxx g++] [--small]

--sanitize builds the program with the address and undefined-behaviour sanitizers (a stand-alone executable with its own main): the
matrix, rows, w, genes, the block, ties, nonzero and the workspace are heap blocks of exactly the stated sizes, so a read or write outside
them is reported.  --small: the first shapes only."""
import argparse
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np

SHIMS = """#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#define __host__
#define __device__
#define __forceinline__ inline
"""
MAIN = """
struct Args { const void* X; long ld; const int* rows; int col_off, u16; int G, n_rows, n_piece, pos_off, n, n_sel;
              const float* w; const int* genes; float* out; long ld_out; long long* ties; int* nonzero; char* ws; };

static void stage_workgroup(const Args& a, int bx, int by) {   // rank_stage_kernel<., true>, wave by wave and lane by lane
  static unsigned tile[RANK_TG][RANK_TP + 1];
  const int p0 = a.pos_off + bx * RANK_TP, p_end = a.pos_off + a.n_piece, j0 = by * RANK_TG;
  for (int wave = 0; wave < 4; ++wave)
    for (int lane = 0; lane < 64; ++lane) {
      const int j = j0 + lane;
      int g = -1;
      if (j < a.n_sel) g = a.genes ? a.genes[j] : j;
      const bool g_ok = g >= 0 && g < a.G;
      for (int pl0 = wave; pl0 < RANK_TP; pl0 += 4 * RANK_UNROLL)
        for (int u = 0; u < RANK_UNROLL; ++u) {   // every load is made, from an address that exists; what does not belong is dropped
          const int q = rank_stage_position(p0 + pl0 + 4 * u, p_end);
          const int r = a.rows ? a.rows[q - a.pos_off] : q - a.pos_off;
          const bool ok = p0 + pl0 + 4 * u < p_end && r >= 0 && r < a.n_rows && g_ok;
          const long at = rank_stage_source(ok, r, a.ld, a.col_off, g_ok ? g : 0);
          const float c = a.u16 ? (float)((const unsigned short*)a.X)[at] : ((const float*)a.X)[at];
          const float wv = a.w ? a.w[q] : 1.f;
          tile[lane][pl0 + 4 * u] = ok ? rank_key_bits(c, wv, a.w != nullptr) : 0u;
        }
    }
  int* const cursor = (int*)(a.ws + rank_ws_cursor_off());
  rank_entry_t* const half_a = (rank_entry_t*)(a.ws + rank_ws_half_off(0, a.n, a.n_sel));
  for (int gl = 0; gl < RANK_TG; ++gl) {
    const int jj = j0 + gl;
    if (jj >= a.n_sel) continue;
    unsigned long long b0 = 0, b1 = 0;
    for (int lane = 0; lane < 64; ++lane) {
      if (tile[gl][lane] != 0u) b0 |= 1ull << lane;
      if (tile[gl][64 + lane] != 0u) b1 |= 1ull << lane;
    }
    const int c0 = rank_popc(b0), cnt = c0 + rank_popc(b1);
    if (cnt == 0) continue;
    const int base = cursor[jj];
    cursor[jj] += cnt;
    rank_entry_t* const col = half_a + (long)jj * a.n;
    for (int lane = 0; lane < 64; ++lane) {   // the position word: p itself (no segment code is read)
      const unsigned k0 = tile[gl][lane], k1 = tile[gl][64 + lane];
      if (k0 != 0u) { const int slot = base + rank_popc(b0 & rank_lanes_below(lane)); if (slot >= 0 && slot < a.n) col[slot] = rank_pos_entry(k0, p0 + lane); }
      if (k1 != 0u) { const int slot = base + c0 + rank_popc(b1 & rank_lanes_below(lane)); if (slot >= 0 && slot < a.n) col[slot] = rank_pos_entry(k1, p0 + 64 + lane); }
    }
  }
}

static int g_paths[2];
static long g_high_positions;
static void values_workgroup(const Args& a, int j) {   // rank_values_kernel
  const int* const cursor = (const int*)(a.ws + rank_ws_cursor_off());
  int m = cursor[j] < 0 ? 0 : cursor[j];
  if (m > a.n) m = a.n;
  const int n_zero = a.n - m;
  rank_entry_t* src = (rank_entry_t*)(a.ws + rank_ws_half_off(0, a.n, a.n_sel)) + (long)j * a.n;
  float* const col = (float*)(a.ws + rank_values_col_off(a.n, a.n_sel)) + (long)j * a.n;
  if (n_zero > 0)
    for (int i = 0; i < a.n; ++i) col[i] = (float)rank_value_zero(n_zero, a.n);
  rank_entry_t* buf = nullptr;
  const rank_entry_t* sorted;
  if (m <= RANK_LDS_CAP) {
    ++g_paths[0];
    const int P = rank_pow2(m);
    buf = (rank_entry_t*)malloc(8 * (size_t)P);
    for (int i = 0; i < P; ++i) buf[i] = i < m ? src[i] : ~0ull;
    for (int k = 2; k <= P; k <<= 1)
      for (int jj = k >> 1; jj > 0; jj >>= 1)
        for (int t = 0; t < (P >> 1); ++t) rank_bitonic_cx(buf, t, jj, k);
    sorted = buf;
  } else {   // (the radix passes are walked by tools/rank_host_check.py: any stable sort by key gives their order)
    ++g_paths[1];
    std::stable_sort(src, src + m, [](rank_entry_t x, rank_entry_t y) { return rank_entry_key(x) < rank_entry_key(y); });
    sorted = src;
  }
  unsigned long long tie = 0;
  for (int i = 0; i < m; ++i) {
    const int s = rank_run_begin(sorted, i), e = rank_run_end(sorted, i, m);
    const unsigned p = rank_entry_seg(sorted[i]);
    if (p > 65535u) ++g_high_positions;
    if (p < (unsigned)a.n) col[p] = (float)rank_value_term(n_zero, s, e, a.n);
    else { fprintf(stderr, "a position word outside the list\\n"); exit(5); }
    if (s == i) tie += rank_tie_term(e - s);
  }
  if (a.ties) a.ties[j] = (long long)(tie + rank_tie_term(n_zero));
  if (a.nonzero) a.nonzero[j] = m;
  free(buf);
}

static void store_workgroup(const Args& a, int bx, int by) {   // rank_values_store_kernel, thread by thread
  static float tile[RANKV_T][RANKV_T + 1];
  const int p0 = bx * RANKV_T, j0 = by * RANKV_T;
  const float* const cols = (const float*)(a.ws + rank_values_col_off(a.n, a.n_sel));
  for (int t = 0; t < RANKV_THREADS; ++t)
    for (int r = 0; r < RANKV_T * RANKV_T / RANKV_THREADS; ++r) {
      const int gl = rank_tr_row(r, t), pl = rank_tr_lane(t);
      tile[gl][pl] = cols[rank_tr_src(rank_tr_clamp(j0 + gl, a.n_sel), rank_tr_clamp(p0 + pl, a.n), a.n)];
    }
  for (int t = 0; t < RANKV_THREADS; ++t)
    for (int r = 0; r < RANKV_T * RANKV_T / RANKV_THREADS; ++r) {
      const int pl = rank_tr_row(r, t), gl = rank_tr_lane(t);
      if (p0 + pl < a.n && j0 + gl < a.n_sel) a.out[rank_tr_dst(p0 + pl, j0 + gl, a.ld_out)] = tile[gl][pl];
    }
}

int main(int argc, char** argv) {   // argv: input file, output file
  if (argc < 3) return 2;
  FILE* f = fopen(argv[1], "rb"); FILE* o = fopen(argv[2], "wb");
  if (!f || !o) return 2;
  int h[12];   // n, n_sel, G, n_rows, ld, col_off, u16, has_w, has_genes, ld_out, (spare)
  if (fread(h, 4, 12, f) != 12) return 3;
  const int n = h[0], n_sel = h[1], G = h[2], n_rows = h[3], ld = h[4], col_off = h[5], u16 = h[6], ld_out = h[9];
  const size_t nx = (size_t)(n_rows - 1) * ld + col_off + G, esz = u16 ? 2 : 4, no = (size_t)(n - 1) * ld_out + n_sel;
  void* X = malloc(nx * esz);
  int* rows = (int*)malloc(4 * (size_t)n); float* w = (float*)malloc(4 * (size_t)n); int* genes = (int*)malloc(4 * (size_t)n_sel);
  float* out = (float*)malloc(4 * no); long long* ties = (long long*)malloc(8 * (size_t)n_sel); int* nonzero = (int*)malloc(4 * (size_t)n_sel);
  if (fread(X, esz, nx, f) != nx || fread(rows, 4, n, f) != (size_t)n || fread(w, 4, n, f) != (size_t)n || fread(genes, 4, n_sel, f) != (size_t)n_sel ||
      fread(out, 4, no, f) != no) return 3;
  const long long bytes = rank_values_ws_bytes(n, n_sel);
  if (bytes <= 0 || bytes % 8 || bytes != ((rank_ws_bytes(n, n_sel) + 4ll * n * n_sel + 7) & ~7ll) || rank_values_col_off(n, n_sel) != rank_ws_bytes(n, n_sel)) return 4;
  char* ws = (char*)malloc(bytes);
  memset(ws, 0xA5, bytes);
  memset(ws, 0, RANK_WS_HEAD);   // rank_reset_kernel
  Args a{X, ld, nullptr, col_off, u16, G, n_rows, 0, 0, n, n_sel, h[7] ? w : nullptr, h[8] ? genes : nullptr, out, ld_out, ties, nonzero, ws};
  const int cut = n / 2;   // two pieces: [0, cut) and [cut, n), each with its own row list and pos_off
  for (int piece = 0; piece < 2; ++piece) {
    a.pos_off = piece ? cut : 0; a.n_piece = piece ? n - cut : cut; a.rows = rows + a.pos_off;
    if (a.n_piece == 0) continue;
    for (int bx = 0; bx < (a.n_piece + RANK_TP - 1) / RANK_TP; ++bx)
      for (int by = 0; by < (n_sel + RANK_TG - 1) / RANK_TG; ++by) stage_workgroup(a, bx, by);
  }
  for (int j = 0; j < n_sel; ++j) values_workgroup(a, j);
  for (int bx = 0; bx < (n + RANKV_T - 1) / RANKV_T; ++bx)
    for (int by = 0; by < (n_sel + RANKV_T - 1) / RANKV_T; ++by) store_workgroup(a, bx, by);
  fwrite(out, 4, no, o); fwrite(ties, 8, n_sel, o); fwrite(nonzero, 4, n_sel, o);
  printf("paths: lds %d sort %d  position words above 65535: %ld\\n", g_paths[0], g_paths[1], g_high_positions);
  printf("rank_values_ws_bytes(%d, %d) = %lld  (0, 5) = %lld  (5, 0) = %lld  (%d, 1) = %lld  (1, %d) = %lld  (3, 1) = %lld\\n", n, n_sel, bytes, rank_values_ws_bytes(0, 5),
         rank_values_ws_bytes(5, 0), RANK_MAX_N + 1, rank_values_ws_bytes(RANK_MAX_N + 1, 1), RANK_SLAB + 1, rank_values_ws_bytes(1, RANK_SLAB + 1), rank_values_ws_bytes(3, 1));
  if (rank_values_ws_bytes(0, 5) || rank_values_ws_bytes(5, 0) || rank_values_ws_bytes(RANK_MAX_N + 1, 1) || rank_values_ws_bytes(1, RANK_SLAB + 1)) return 6;
  if (rank_values_ws_bytes(3, 1) != RANK_WS_HEAD + 48 + 16) return 6;   // 12 bytes of column, rounded up to 16
  free(ws); free(nonzero); free(ties); free(out); free(genes); free(w); free(rows); free(X); fclose(o); fclose(f);
  return 0;
}
"""
# (n, n_rows, G, ld, col_off, n_sel (0 = all genes, no list), dtype, weights, density, ld_out - n_sel)
SHAPES = [(1, 3, 5, 7, 1, 0, "u16", False, 0.5, 0), (2, 4, 9, 9, 0, 4, "f32", True, 0.7, 2), (127, 60, 70, 75, 3, 66, "u16", True, 0.3, 1),
          (129, 200, 65, 65, 0, 0, "u16", False, 0.2, 0), (300, 300, 12, 16, 2, 12, "f32", True, 1.0, 3),
          (8400, 8400, 5, 5, 0, 0, "u16", False, 1.0, 2), (70001, 5000, 3, 4, 1, 3, "f32", True, 0.97, 1)]
SENTINEL = np.float32(-12345.0)


def host_source() -> str:
    """both cores as they stand in the headers, between the stand-ins and the driver"""
    csrc = os.path.join(ROOT, "spvipes_amd", "csrc")
    rank, values = open(os.path.join(csrc, "spv_rank.h")).read(), open(os.path.join(csrc, "spv_rank_values.h")).read()
    return (SHIMS + rank[rank.index("// ---- RANK-CORE-BEGIN ----"):rank.index("// ---- RANK-CORE-END ----")]
            + values[values.index("// ---- RANK-VALUES-CORE-BEGIN ----"):values.index("// ---- RANK-VALUES-CORE-END ----")] + MAIN)


def reference(keys: np.ndarray):
    """keys fp32 [n, n_sel] -> (block int64 [n, n_sel] = L + U - n, ties int64 [n_sel], nonzero [n_sel]) by a plain sort and two counts per key"""
    n, n_sel = keys.shape
    block, ties = np.zeros((n, n_sel), np.int64), np.zeros(n_sel, np.int64)
    for j in range(n_sel):
        s = np.sort(keys[:, j])
        block[:, j] = np.searchsorted(s, keys[:, j], "left").astype(np.int64) + np.searchsorted(s, keys[:, j], "right").astype(np.int64) - n
        t = np.unique(s, return_counts=True)[1].astype(np.int64)
        ties[j] = (t ** 3 - t).sum()
    return block, ties, (keys != 0).sum(0)


def make_case(rng, n, n_rows, G, ld, col_off, n_sel, dtype, density):
    if dtype == "u16":
        x = rng.integers(0, 65536, (n_rows, ld)).astype(np.uint16)
        x[:, col_off:col_off + G] = (rng.integers(1, 6, (n_rows, G)) * (rng.random((n_rows, G)) < density)).astype(np.uint16)
        if G > 2:
            x[:, col_off + 1] = np.arange(n_rows) % 65535 + 1   # (nearly) all distinct
            x[:, col_off + 2] = 7                               # all equal
    else:
        x = rng.random((n_rows, ld)).astype(np.float32)
        x[:, col_off:col_off + G] = (np.round(rng.gamma(1.0, 3.0, (n_rows, G)) * 4) / 4 * (rng.random((n_rows, G)) < density)).astype(np.float32)
    rows = rng.integers(0, n_rows, n).astype(np.int32)
    if n > 3:
        rows[1], rows[2] = -1, n_rows   # outside the matrix: read as zero keys, never dereferenced
    w = (rng.random(n) * 3).astype(np.float32)
    w[rng.random(n) < 0.1] = 0.0
    genes = (rng.integers(0, G, n_sel) if n_sel else np.arange(G)).astype(np.int32)
    return x, rows, w, genes


def run(shapes, sanitize=False, cxx="g++", verbose=True) -> int:
    bad = 0
    rng = np.random.default_rng(29)
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "spearman_host.cpp"), os.path.join(d, "spearman_host")
        open(src, "w").write(host_source())
        subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", *(["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []),
                        "-o", exe, src], check=True)
        for n, n_rows, G, ld, col_off, n_sel, dtype, weights, density, extra in shapes:
            x, rows, w, genes = make_case(rng, n, n_rows, G, ld, col_off, n_sel, dtype, density)
            ns = n_sel or G
            ld_out = ns + extra
            nx, no = (n_rows - 1) * ld + col_off + G, (n - 1) * ld_out + ns
            fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
            with open(fin, "wb") as f:
                f.write(np.array([n, ns, G, n_rows, ld, col_off, dtype == "u16", weights, bool(n_sel), ld_out, 0, 0], np.int32).tobytes() + x.ravel()[:nx].tobytes()
                        + rows.tobytes() + w.tobytes() + genes.tobytes() + np.full(no, SENTINEL, np.float32).tobytes())
            res = subprocess.run([exe, fin, fout], check=True, capture_output=True, text=True)
            raw = np.fromfile(fout, np.uint8)
            flat = np.full(n * ld_out, SENTINEL, np.float32)
            flat[:no] = raw[:4 * no].view(np.float32)
            got = flat.reshape(n, ld_out)
            got_t, got_m = raw[4 * no:4 * no + 8 * ns].view(np.int64), raw[4 * no + 8 * ns:].view(np.int32)
            ok_row = (rows >= 0) & (rows < n_rows)
            c = np.where(ok_row[:, None], x[np.where(ok_row, rows, 0)][:, col_off:col_off + G][:, genes].astype(np.float32), np.float32(0))
            keys = c * w[:, None] if weights else c
            assert keys.dtype == np.float32
            want, want_t, want_m = reference(keys)
            high = int(res.stdout.split("above 65535:")[1].split()[0])
            ok = [bool((got[:, :ns].astype(np.int64) == want).all() and (got[:, :ns] == np.round(got[:, :ns])).all()), bool((got_t == want_t).all()),
                  bool((got_m == want_m).all()), bool((got[:, ns:] == SENTINEL).all()), n <= 65536 or high > 0]
            bad += not all(ok)
            if verbose:
                print(f"n {n:6d} genes {ns:3d} {dtype} {'weighted' if weights else 'raw     '}  block {'ok' if ok[0] else 'DIFFERS'}  ties {'ok' if ok[1] else 'DIFFER'}"
                      f"  nonzero {'ok' if ok[2] else 'DIFFERS'}  columns >= n_sel {'ok' if ok[3] else 'TOUCHED'}  {res.stdout.splitlines()[0]}")
        if verbose:
            print(res.stdout.splitlines()[1])
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sanitize", action="store_true")
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--cxx", default="g++")
    a = ap.parse_args()
    bad = run(SHAPES[:5] if a.small else SHAPES, a.sanitize, a.cxx)
    print("all equal" if not bad else f"{bad} shape(s) DIFFER")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
