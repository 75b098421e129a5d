#!/usr/bin/env python3
"""The rank-sum kernels' core on the CPU: compiles the text between the RANK-CORE marks of csrc/spv_rank.h -- the key image, the entry
packing, the bitonic compare-exchange map, the digit and same-digit-lanes maps of the radix passes, the tie-run walk with L, U and
t^3 - t, the zero-run accounting and the workspace layout and size, exactly as the kernels use them -- as plain C++, with a driver that
walks the grids the way rank_stage_kernel / rank_sums_kernel do: 4 emulated waves of 64 lanes per stage workgroup with the ballots taken
over the lanes, the LDS tile and histogram, the gene cursors; RANK_WAVES emulated waves per sums workgroup, the bitonic network step by
step, the radix passes tile by tile with their (wave, digit) tables and guarded stores.  The list is staged in TWO pieces whenever it has
two positions (pos_off > 0 is exercised).  Whole tables are then compared with numpy for EQUALITY:

  * rank2 and ties must equal a plain sort-and-count reference on numpy float32 keys;
  * columns >= n_sel of rank2 must keep their sentinel.
No GPU, nothing loaded into Python.  It checks everything except the hardware's atomics, ballots and barriers themselves.

    python tools/rank_host_check.py [--sanitize] [--cxx g++] [--small]

--sanitize builds the program with the address and undefined-behaviour sanitizers (a stand-alone executable with its own main): the
matrix, rows, seg, w, genes, rank2, ties, the workspace and the LDS sort buffer are heap blocks of exactly the stated sizes (the matrix
ends with its last row's last gene, the workspace has spv_rank_ws_bytes(n, n_sel) bytes, the sort buffer the power of two the network
runs over), so a read or write outside them is reported.  --small: the first shapes only."""
import argparse
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np

SHIMS = """#include <cstdio>
#include <cstdlib>
#include <cstring>
#define __host__
#define __device__
#define __forceinline__ inline
"""
MAIN = """
struct Args { const void* X; long ld; const int* rows; int col_off, u16; int G, n_rows, n_piece, pos_off, n, n_seg, n_sel;
              const int* seg; const float* w; const int* genes; long long* rank2; long ld_rank2; long long* ties; char* ws; };

static void stage_workgroup(const Args& a, int bx, int by) {   // rank_stage_kernel, wave by wave and lane by lane
  static unsigned tile[RANK_TG][RANK_TP + 1];
  static int hist[RANK_MAX_SEG];
  const int p0 = a.pos_off + bx * RANK_TP, p_end = a.pos_off + a.n_piece, j0 = by * RANK_TG;
  const bool count_segments = by == 0;
  if (count_segments) memset(hist, 0, sizeof(hist));
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
  int code[2][64]; bool live[2][64];
  for (int c = 0; c < 2; ++c)
    for (int lane = 0; lane < 64; ++lane) {
      const int p = p0 + 64 * c + lane;
      live[c][lane] = p < p_end;
      code[c][lane] = live[c][lane] ? a.seg[p] : -1;
    }
  if (count_segments)
    for (int c = 0; c < 2; ++c)
      for (int lane = 0; lane < 64; ++lane)
        if (live[c][lane] && code[c][lane] >= 0 && code[c][lane] < a.n_seg) ++hist[code[c][lane]];
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
    for (int lane = 0; lane < 64; ++lane) {
      const unsigned k0 = tile[gl][lane], k1 = tile[gl][64 + lane];
      if (k0 != 0u) { const int slot = base + rank_popc(b0 & rank_lanes_below(lane)); if (slot >= 0 && slot < a.n) col[slot] = rank_entry(k0, code[0][lane], a.n_seg); }
      if (k1 != 0u) { const int slot = base + c0 + rank_popc(b1 & rank_lanes_below(lane)); if (slot >= 0 && slot < a.n) col[slot] = rank_entry(k1, code[1][lane], a.n_seg); }
    }
  }
  if (count_segments) {
    int* const segcnt = (int*)(a.ws + rank_ws_segcnt_off());
    for (int k = 0; k < a.n_seg; ++k) segcnt[k] += hist[k];
  }
}

static int g_paths[2];
static void sums_workgroup(const Args& a, int j) {   // rank_sums_kernel
  const int* const cursor = (const int*)(a.ws + rank_ws_cursor_off());
  const int* const segcnt = (const int*)(a.ws + rank_ws_segcnt_off());
  int m = cursor[j] < 0 ? 0 : cursor[j];
  if (m > a.n) m = a.n;
  const int n_zero = a.n - m;
  rank_entry_t* src = (rank_entry_t*)(a.ws + rank_ws_half_off(0, a.n, a.n_sel)) + (long)j * a.n;
  rank_entry_t* dst = (rank_entry_t*)(a.ws + rank_ws_half_off(1, a.n, a.n_sel)) + (long)j * a.n;
  unsigned long long* acc = (unsigned long long*)calloc(a.n_seg, 8);
  int* stored = (int*)calloc(a.n_seg, 4);
  unsigned long long tie = 0;
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
  } else {
    ++g_paths[1];
    static unsigned hist[4][256], wavecnt[RANK_WAVES][256], run[256];
    memset(hist, 0, sizeof(hist));
    for (int i = 0; i < m; ++i)
      for (int ps = 0; ps < 4; ++ps) ++hist[ps][rank_digit(rank_entry_key(src[i]), ps)];
    for (int ps = 0; ps < 4; ++ps) {
      bool skip = false;
      for (int d = 0; d < 256; ++d) skip = skip || hist[ps][d] == (unsigned)m;
      if (skip) continue;
      for (int d = 0, s = 0; d < 256; ++d) { run[d] = s; s += hist[ps][d]; }
      for (int t0 = 0; t0 < m; t0 += RANK_THREADS) {
        static int before[RANK_THREADS];
        memset(wavecnt, 0, sizeof(wavecnt));
        for (int wave = 0; wave < RANK_WAVES; ++wave) {
          unsigned long long bal[8] = {0}, valid = 0;
          unsigned d[64];
          for (int lane = 0; lane < 64; ++lane) {
            const int i = t0 + 64 * wave + lane;
            const rank_entry_t e = i < m ? src[i] : 0ull;
            d[lane] = rank_digit(rank_entry_key(e), ps);
            if (i < m) valid |= 1ull << lane;
            for (int b = 0; b < 8; ++b) if ((d[lane] >> b) & 1u) bal[b] |= 1ull << lane;
          }
          for (int lane = 0; lane < 64; ++lane) {
            const unsigned long long peers = rank_peers(bal, d[lane], valid);
            before[64 * wave + lane] = rank_popc(peers & rank_lanes_below(lane));
            if (((valid >> lane) & 1ull) && before[64 * wave + lane] == 0) wavecnt[wave][d[lane]] = (unsigned)rank_popc(peers);
          }
        }
        for (int d = 0; d < 256; ++d) {
          unsigned s = run[d];
          for (int w = 0; w < RANK_WAVES; ++w) { const unsigned c = wavecnt[w][d]; wavecnt[w][d] = s; s += c; }
          run[d] = s;
        }
        for (int tid = 0; tid < RANK_THREADS; ++tid) {
          const int i = t0 + tid;
          if (i >= m) continue;
          const unsigned at = wavecnt[tid >> 6][rank_digit(rank_entry_key(src[i]), ps)] + (unsigned)before[tid];
          if (at < (unsigned)m) dst[at] = src[i];
          else { fprintf(stderr, "scatter outside the column\\n"); exit(5); }
        }
      }
      rank_entry_t* const t = src; src = dst; dst = t;
    }
    sorted = src;
  }
  for (int i = 0; i < m; ++i) {
    const int s = rank_run_begin(sorted, i), e = rank_run_end(sorted, i, m);
    const unsigned sg = rank_entry_seg(sorted[i]);
    if (sg < (unsigned)a.n_seg) { acc[sg] += rank_elem_term(n_zero, s, e); ++stored[sg]; }
    if (s == i) tie += rank_tie_term(e - s);
  }
  for (int k = 0; k < a.n_seg; ++k) a.rank2[(long)k * a.ld_rank2 + j] = (long long)(acc[k] + rank_zero_term(segcnt[k], stored[k], n_zero));
  a.ties[j] = (long long)(tie + rank_tie_term(n_zero));
  free(buf); free(stored); free(acc);
}

int main(int argc, char** argv) {   // argv: input file, output file
  if (argc < 3) return 2;
  FILE* f = fopen(argv[1], "rb"); FILE* o = fopen(argv[2], "wb");
  if (!f || !o) return 2;
  int h[12];   // n, n_seg, n_sel, G, n_rows, ld, col_off, u16, has_w, has_genes, ld_rank2, (spare)
  if (fread(h, 4, 12, f) != 12) return 3;
  const int n = h[0], n_seg = h[1], n_sel = h[2], G = h[3], n_rows = h[4], ld = h[5], col_off = h[6], u16 = h[7], ld_rank2 = h[10];
  const size_t nx = (size_t)(n_rows - 1) * ld + col_off + G, esz = u16 ? 2 : 4, nr = (size_t)(n_seg - 1) * ld_rank2 + n_sel;
  void* X = malloc(nx * esz);
  int* rows = (int*)malloc(4 * (size_t)n); int* seg = (int*)malloc(4 * (size_t)n); float* w = (float*)malloc(4 * (size_t)n);
  int* genes = (int*)malloc(4 * (size_t)n_sel);
  long long* rank2 = (long long*)malloc(8 * nr); long long* ties = (long long*)malloc(8 * (size_t)n_sel);
  if (fread(X, esz, nx, f) != nx || fread(rows, 4, n, f) != (size_t)n || fread(seg, 4, n, f) != (size_t)n || fread(w, 4, n, f) != (size_t)n ||
      fread(genes, 4, n_sel, f) != (size_t)n_sel || fread(rank2, 8, nr, f) != nr) return 3;
  const long long bytes = rank_ws_bytes(n, n_sel);
  if (bytes <= 0 || bytes % 8) return 4;
  char* ws = (char*)malloc(bytes);
  memset(ws, 0xA5, bytes);
  memset(ws, 0, RANK_WS_HEAD);   // rank_reset_kernel
  Args a{X, ld, nullptr, col_off, u16, G, n_rows, 0, 0, n, n_seg, n_sel, seg, h[8] ? w : nullptr, h[9] ? genes : nullptr, rank2, ld_rank2, ties, ws};
  const int cut = n / 2;   // two pieces: [0, cut) and [cut, n), each with its own row list and pos_off
  for (int piece = 0; piece < 2; ++piece) {
    a.pos_off = piece ? cut : 0; a.n_piece = piece ? n - cut : cut; a.rows = rows + a.pos_off;
    if (a.n_piece == 0) continue;
    for (int bx = 0; bx < (a.n_piece + RANK_TP - 1) / RANK_TP; ++bx)
      for (int by = 0; by < (n_sel + RANK_TG - 1) / RANK_TG; ++by) stage_workgroup(a, bx, by);
  }
  for (int j = 0; j < n_sel; ++j) sums_workgroup(a, j);
  fwrite(rank2, 8, nr, o); fwrite(ties, 8, n_sel, o);
  printf("paths: lds %d radix %d\\n", g_paths[0], g_paths[1]);
  printf("rank_ws_bytes(%d, %d) = %lld  (0, 5) = %lld  (5, 0) = %lld  (%d, 1) = %lld  (1, %d) = %lld\\n", n, n_sel, bytes, rank_ws_bytes(0, 5), rank_ws_bytes(5, 0),
         RANK_MAX_N + 1, rank_ws_bytes(RANK_MAX_N + 1, 1), RANK_SLAB + 1, rank_ws_bytes(1, RANK_SLAB + 1));
  free(ws); free(ties); free(rank2); free(genes); free(w); free(seg); free(rows); free(X); fclose(o); fclose(f);
  return 0;
}
"""
# (n, n_rows, G, ld, col_off, n_sel (0 = all genes, no list), n_seg, dtype, weights, density, ld_rank2 - n_sel)
SHAPES = [(1, 3, 5, 7, 1, 0, 1, "u16", False, 0.5, 0), (2, 4, 9, 9, 0, 4, 3, "f32", True, 0.7, 2), (127, 60, 70, 75, 3, 66, 5, "u16", True, 0.3, 1),
          (129, 200, 65, 65, 0, 0, 1024, "u16", False, 0.2, 0), (300, 300, 12, 16, 2, 12, 4, "f32", True, 1.0, 3),
          (8400, 8400, 5, 5, 0, 0, 3, "u16", False, 1.0, 2), (9000, 5000, 6, 8, 1, 6, 7, "u16", True, 1.0, 0), (20000, 20000, 3, 4, 0, 3, 20, "f32", True, 0.97, 0)]


def host_source() -> str:
    """the core as it stands in the header, between the stand-ins and the driver"""
    src = open(os.path.join(ROOT, "spvipes_amd", "csrc", "spv_rank.h")).read()
    return SHIMS + src[src.index("// ---- RANK-CORE-BEGIN ----"):src.index("// ---- RANK-CORE-END ----")] + MAIN


def reference(keys: np.ndarray, seg: np.ndarray, n_seg: int):
    """keys fp32 [n, n_sel] -> (rank2 int64 [n_seg, n_sel], ties int64 [n_sel]) by a plain sort and two counts per key"""
    n, n_sel = keys.shape
    rank2, ties = np.zeros((n_seg, n_sel), np.int64), np.zeros(n_sel, np.int64)
    inside = (seg >= 0) & (seg < n_seg)
    for j in range(n_sel):
        s = np.sort(keys[:, j])
        term = np.searchsorted(s, keys[:, j], "left").astype(np.int64) + np.searchsorted(s, keys[:, j], "right").astype(np.int64) + 1
        np.add.at(rank2[:, j], seg[inside], term[inside])
        t = np.unique(s, return_counts=True)[1].astype(np.int64)
        ties[j] = (t ** 3 - t).sum()
    return rank2, ties


def make_case(rng, n, n_rows, G, ld, col_off, n_sel, n_seg, dtype, weights, density):
    if dtype == "u16":
        x = rng.integers(0, 65536, (n_rows, ld)).astype(np.uint16)
        x[:, col_off:col_off + G] = (rng.integers(1, 6, (n_rows, G)) * (rng.random((n_rows, G)) < density)).astype(np.uint16)
        if G > 2:
            x[:, col_off + 1] = np.arange(n_rows) % 65535 + 1 if n_rows < 65535 else rng.integers(1, 65536, n_rows)   # (nearly) all distinct
            x[:, col_off + 2] = 7                                                                                       # all equal
    else:
        x = rng.random((n_rows, ld)).astype(np.float32)
        x[:, col_off:col_off + G] = (np.round(rng.gamma(1.0, 3.0, (n_rows, G)) * 4) / 4 * (rng.random((n_rows, G)) < density)).astype(np.float32)
    rows = rng.integers(0, n_rows, n).astype(np.int32)
    if n > 3:
        rows[1], rows[2] = -1, n_rows   # outside the matrix: read as zero counts, never dereferenced
    seg = rng.integers(-1, n_seg + 1, n).astype(np.int32)   # -1 and n_seg: ranked, counted in no sum
    w = (rng.random(n) * 3).astype(np.float32)
    w[rng.random(n) < 0.1] = 0.0
    genes = (rng.integers(0, G, n_sel) if n_sel else np.arange(G)).astype(np.int32)
    return x, rows, seg, w, genes


def run(shapes, sanitize=False, cxx="g++", verbose=True) -> int:
    bad = 0
    rng = np.random.default_rng(27)
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "rank_host.cpp"), os.path.join(d, "rank_host")
        open(src, "w").write(host_source())
        subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", *(["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []),
                        "-o", exe, src], check=True)
        for n, n_rows, G, ld, col_off, n_sel, n_seg, dtype, weights, density, extra in shapes:
            x, rows, seg, w, genes = make_case(rng, n, n_rows, G, ld, col_off, n_sel, n_seg, dtype, weights, density)
            ns = n_sel or G
            ld_rank2 = ns + extra
            table = np.full((n_seg, ld_rank2), -77, np.int64)
            nx, nr = (n_rows - 1) * ld + col_off + G, (n_seg - 1) * ld_rank2 + ns
            fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
            with open(fin, "wb") as f:
                f.write(np.array([n, n_seg, ns, G, n_rows, ld, col_off, dtype == "u16", weights, bool(n_sel), ld_rank2, 0], np.int32).tobytes() + x.ravel()[:nx].tobytes()
                        + rows.tobytes() + seg.tobytes() + w.tobytes() + genes.tobytes() + table.ravel()[:nr].tobytes())
            res = subprocess.run([exe, fin, fout], check=True, capture_output=True, text=True)
            out = np.fromfile(fout, np.int64)
            flat = np.full(n_seg * ld_rank2, -77, np.int64)
            flat[:nr] = out[:nr]
            got, got_t = flat.reshape(n_seg, ld_rank2), out[nr:]
            ok_row = (rows >= 0) & (rows < n_rows)
            c = np.where(ok_row[:, None], x[np.where(ok_row, rows, 0)][:, col_off:col_off + G][:, genes].astype(np.float32), np.float32(0))
            keys = c * w[:, None] if weights else c
            assert keys.dtype == np.float32
            want, want_t = reference(keys, seg, n_seg)
            ok = [bool((got[:, :ns] == want).all()), bool((got_t == want_t).all()), bool((got[:, ns:] == -77).all())]
            bad += not all(ok)
            if verbose:
                print(f"n {n:6d} genes {ns:3d} segments {n_seg:4d} {dtype} {'weighted' if weights else 'raw     '}  rank2 {'ok' if ok[0] else 'DIFFERS'}  ties {'ok' if ok[1] else 'DIFFER'}"
                      f"  columns >= n_sel {'ok' if ok[2] else 'TOUCHED'}  {res.stdout.splitlines()[0]}")
        if verbose:
            print(res.stdout.splitlines()[1])
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sanitize", action="store_true")
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--cxx", default="g++")
    a = ap.parse_args()
    bad = run(SHAPES[:6] if a.small else SHAPES, a.sanitize, a.cxx)
    print("all equal" if not bad else f"{bad} shape(s) DIFFER")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
