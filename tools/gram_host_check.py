#!/usr/bin/env python3
"""The Gram kernel's core on the CPU: compiles the text between the GRAM-CORE marks of csrc/spv_gram.h -- the triangle index -> tile map,
the slab plan and bounds, the staging map and its guarded load, the lane -> operand and lane -> result maps of the f64 MFMA, the add with
its mirror, the merge order and the workspace layout and size, exactly as the kernels use them -- as plain C++, with a driver that walks
the grid the way gram_partial_kernel / gram_merge_kernel do: 256 emulated threads per workgroup, 64 emulated lanes per wave, and a plain
loop in place of v_mfma_f64_16x16x4_f64 (A[i][k] from lane 16 k + i, B[k][j] from lane 16 k + j, k ascending).  Whole tables are then
compared with numpy:

  * lattice inputs (integer-valued fp32, every sum below 2^53) must EQUAL the int64 reference bit for bit -- a wrong lane map, tile map,
    mirror address or slab bound shows here;
  * real inputs must lie within gamma_m (|start| + sum |x_i x_j|) of long-double sums of the exact products, m = n_use + slabs + 1;
  * both triangles must agree bit for bit, columns >= n of the table must keep their sentinel, and uncounted rows / padding columns of
    x hold NaN that must never arrive in a sum.
No GPU, nothing loaded into Python.  It checks everything except the MFMA instruction itself and the hardware's order inside one.

    python tools/gram_host_check.py [--sanitize] [--cxx g++] [--small]

--sanitize builds the program with the address and undefined-behaviour sanitizers (a stand-alone executable with its own main): x, rows,
sums, gram, the workspace and the LDS panels are heap blocks of exactly the stated sizes (x ends with its last row's n-th column), so a
read or write outside them is reported.  --small: the first shapes only."""
import argparse
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np

SHIMS = """#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#define __host__
#define __device__
#define __forceinline__ inline
"""
MAIN = """
// the MFMA's stand-in over the 64 lanes of a wave: D = A B + C with A[i][k] in lane 16 k + i, B[k][j] in lane 16 k + j (one double each)
static void mfma_f64_16x16x4(const double* a, const double* b, double (*acc)[4]) {
  for (int lane = 0; lane < 64; ++lane)
    for (int reg = 0; reg < 4; ++reg) {
      const int i = gram_result_row(lane, reg), j = gram_result_col(lane);
      double s = acc[lane][reg];
      for (int k = 0; k < 4; ++k) s += a[16 * k + i] * b[16 * k + j];
      acc[lane][reg] = s;
    }
}

struct Args { const float* x; long ld_x; int n_rows; const int* rows; int n_use, n; double* sums; double* gram; long ld_gram; double* ws; int slabs, per, nt, tiles; };

static void partial_workgroup(const Args& a, int tile, int slab) {   // gram_partial_kernel, thread by thread
  double* panels = (double*)malloc(sizeof(double) * 2 * GRAM_PANEL);
  for (int e = 0; e < 2 * GRAM_PANEL; ++e) panels[e] = NAN;          // what is never staged is never read: a NaN would show
  int ti, tj;
  gram_tile_of(tile, a.nt, ti, tj);
  const bool diag = ti == tj;
  const int r_lo = slab * a.per, r_hi = r_lo + a.per < a.n_use ? r_lo + a.per : a.n_use;
  const int chunks = r_hi > r_lo ? (r_hi - r_lo + GRAM_KC - 1) / GRAM_KC : 0;
  const double* pI = panels;
  const double* pJ = diag ? panels : panels + GRAM_PANEL;
  static double acc[4][2][2][64][4];
  memset(acc, 0, sizeof(acc));
  double colsum[64] = {0};
  static float v[GRAM_THREADS][GRAM_KC / 2];
  auto load = [&](int r0) {
    for (int t = 0; t < GRAM_THREADS; ++t) {
      const int panel = gram_stage_panel(t);
      if (diag && panel) continue;
      const int gcol = (panel ? tj : ti) * GRAM_T + gram_stage_col(t);
      for (int m = 0; m < GRAM_KC / 2; ++m) v[t][m] = gram_load(a.x, a.ld_x, gram_source_row(a.rows, a.n_rows, r0 + gram_stage_row(t, m), r_hi), gcol, a.n);
    }
  };
  load(r_lo);
  for (int c = 0; c < chunks; ++c) {
    for (int t = 0; t < GRAM_THREADS; ++t) {
      const int panel = gram_stage_panel(t);
      if (diag && panel) continue;
      const int gcol = (panel ? tj : ti) * GRAM_T + gram_stage_col(t);
      for (int m = 0; m < GRAM_KC / 2; ++m)
        panels[panel * GRAM_PANEL + gram_stage_row(t, m) * GRAM_LDP + gram_stage_col(t)] =
            gram_counts(r_lo + c * GRAM_KC + gram_stage_row(t, m), r_hi, gcol, a.n) ? (double)v[t][m] : 0.0;
    }
    load(r_lo + (c + 1) * GRAM_KC);
    for (int wave = 0; wave < 4; ++wave) {
      if (!gram_wave_works(wave, diag)) continue;
      const int wr = gram_wave_row(wave), wc = gram_wave_col(wave);
      for (int ks = 0; ks < GRAM_KC / 4; ++ks) {
        double a0[64], a1[64], b0[64], b1[64];
        for (int lane = 0; lane < 64; ++lane) {
          a0[lane] = pI[gram_operand(lane, ks, 32 * wr)], a1[lane] = pI[gram_operand(lane, ks, 32 * wr + 16)];
          b0[lane] = pJ[gram_operand(lane, ks, 32 * wc)], b1[lane] = pJ[gram_operand(lane, ks, 32 * wc + 16)];
        }
        mfma_f64_16x16x4(a0, b0, acc[wave][0][0]); mfma_f64_16x16x4(a0, b1, acc[wave][0][1]);
        mfma_f64_16x16x4(a1, b0, acc[wave][1][0]); mfma_f64_16x16x4(a1, b1, acc[wave][1][1]);
      }
    }
    if (diag)
      for (int lane = 0; lane < 64; ++lane)
        for (int r = 0; r < GRAM_KC; ++r) colsum[lane] += pI[r * GRAM_LDP + lane];
  }
  const bool direct = a.slabs == 1;
  double* part = direct ? nullptr : a.ws + gram_ws_tile(slab, tile, a.tiles);
  for (int wave = 0; wave < 4; ++wave)
    for (int lane = 0; lane < 64; ++lane)
      for (int fi = 0; fi < 2; ++fi)
        for (int fj = 0; fj < 2; ++fj)
          for (int reg = 0; reg < 4; ++reg) {
            const int lr = 32 * gram_wave_row(wave) + 16 * fi + gram_result_row(lane, reg), lc = 32 * gram_wave_col(wave) + 16 * fj + gram_result_col(lane);
            if (direct) gram_add(a.gram, a.ld_gram, a.n, ti * GRAM_T + lr, tj * GRAM_T + lc, acc[wave][fi][fj][lane][reg]);
            else part[lr * GRAM_T + lc] = acc[wave][fi][fj][lane][reg];
          }
  if (diag)
    for (int lane = 0; lane < 64; ++lane) {
      const int j = ti * GRAM_T + lane;
      if (direct) { if (j < a.n) a.sums[j] += colsum[lane]; }
      else a.ws[gram_ws_sums(slab, a.slabs, a.nt, a.tiles) + j] = colsum[lane];
    }
  free(panels);
}

static void merge_workgroup(const Args& a, int tile) {   // gram_merge_kernel
  int ti, tj;
  gram_tile_of(tile, a.nt, ti, tj);
  const long st = (long)a.tiles * (GRAM_T * GRAM_T);
  const double* part = a.ws + gram_ws_tile(0, tile, a.tiles);
  for (int by = 0; by < GRAM_T * GRAM_T / GRAM_THREADS; ++by)   // the grid's second axis: one element per thread
    for (int tid = 0; tid < GRAM_THREADS; ++tid) {
      const int e = tid + GRAM_THREADS * by, lr = e >> 6, lc = e & 63;
      const int i = ti * GRAM_T + lr, j = tj * GRAM_T + lc;
      if (i < a.n && j < a.n && i <= j) gram_add(a.gram, a.ld_gram, a.n, i, j, gram_merge(part + e, st, a.slabs));
      if (ti == tj && by == 0 && tid < GRAM_T) {
        const int jj = ti * GRAM_T + tid;
        if (jj < a.n) a.sums[jj] += gram_merge(a.ws + gram_ws_sums(0, a.slabs, a.nt, a.tiles) + jj, (long)a.nt * GRAM_T, a.slabs);
      }
    }
}

int main(int argc, char** argv) {   // argv: input file, output file
  if (argc < 3) return 2;
  FILE* f = fopen(argv[1], "rb"); FILE* o = fopen(argv[2], "wb");
  if (!f || !o) return 2;
  int h[6];   // n_rows, ld_x, n, n_use (-1: rows = NULL), ld_gram, slabs (0: the plan's)
  if (fread(h, 4, 6, f) != 6) return 3;
  const int n_rows = h[0], ld_x = h[1], n = h[2], ld_gram = h[4];
  const bool listed = h[3] >= 0;
  const int n_use = listed ? h[3] : n_rows;
  const size_t nx = n_rows ? (size_t)(n_rows - 1) * ld_x + n : 0, ng = (size_t)(n - 1) * ld_gram + n;   // exactly what the contract lets be touched
  float* x = (float*)malloc(4 * (nx ? nx : 1));
  int* rows = (int*)malloc(4 * (n_use ? n_use : 1));
  double* sums = (double*)malloc(8 * n);
  double* gram = (double*)malloc(8 * ng);
  if (fread(x, 4, nx, f) != nx || (listed && fread(rows, 4, n_use, f) != (size_t)n_use)) return 3;
  if (fread(sums, 8, n, f) != (size_t)n || fread(gram, 8, ng, f) != ng) return 3;
  const int slabs = h[5] > 0 ? h[5] : gram_slabs(n, n_use);
  const long long wsn = gram_ws_doubles(n, slabs);
  printf("slabs %d\\n", slabs);
  double* ws = (double*)malloc(8 * (wsn ? wsn : 1));
  for (long long e = 0; e < wsn; ++e) ws[e] = NAN;
  const int nt = gram_tiles(n), tiles = gram_tri_tiles(nt);
  const Args a{x, ld_x, n_rows, listed ? rows : nullptr, n_use, n, sums, gram, ld_gram, ws, slabs, gram_slab_rows(n_use > 0 ? n_use : 1, slabs), nt, tiles};
  if (n_use > 0) {
    for (int slab = 0; slab < slabs; ++slab)
      for (int t = 0; t < tiles; ++t) partial_workgroup(a, t, slab);
    if (slabs > 1)
      for (int t = 0; t < tiles; ++t) merge_workgroup(a, t);
  }
  fwrite(sums, 8, n, o); fwrite(gram, 8, ng, o);
  const int shapes[][2] = {{64, 4096}, {130, 257}, {17, 70}, {24, 40}, {1984, 4096}, {2048, 4096}, {4096, 4096}, {1, 0}, {4097, 100}};
  for (auto& s : shapes) printf("gram_slabs(%d, %d) = %d  gram_ws_bytes = %lld\\n", s[0], s[1], gram_slabs(s[0], s[1]), gram_ws_bytes(s[0], s[1]));
  int ti, tj, seen = 0;   // the triangle map is a bijection onto ti <= tj, row by row
  for (int nt2 = 1; nt2 <= 64; ++nt2)
    for (int t = 0, wi = 0, wj = 0; t < gram_tri_tiles(nt2); ++t) {
      gram_tile_of(t, nt2, ti, tj);
      if (ti != wi || tj != wj) ++seen;
      if (++wj == nt2) { ++wi; wj = wi; }
    }
  printf("gram_tile_of: %d mismatches over nt = 1 .. 64\\n", seen);
  free(ws); free(gram); free(sums); free(rows); free(x); fclose(o); fclose(f);
  return seen ? 4 : 0;
}
"""
# (n_rows, ld_x, n, counted rows: None = NULL | "arange" | int (that many, a random ascending subset), ld_gram, slabs (0 = plan), data, start)
SHAPES = [(5, 3, 1, None, 1, 0, "lattice", "zero"), (33, 20, 17, 9, 19, 0, "lattice", "lattice"), (70, 17, 17, None, 17, 0, "lattice", "zero"),
          (257, 131, 130, "arange", 133, 0, "lattice", "lattice"), (40, 70, 65, 31, 65, 3, "real", "real"), (100, 64, 64, None, 64, 0, "real", "zero"),
          (300, 200, 193, 257, 200, 0, "lattice", "zero"), (96, 130, 129, 64, 129, 5, "real", "real"), (4, 16, 15, 1, 16, 0, "real", "zero")]


def host_source() -> str:
    """the core as it stands in the header, between the stand-ins and the driver"""
    src = open(os.path.join(ROOT, "spvipes_amd", "csrc", "spv_gram.h")).read()
    return SHIMS + src[src.index("// ---- GRAM-CORE-BEGIN ----"):src.index("// ---- GRAM-CORE-END ----")] + MAIN


def make_case(rng, n_rows, ld_x, n, counted, ld_gram, data, start):
    if data == "lattice":
        x = rng.integers(-1024, 1025, (n_rows, ld_x)).astype(np.float32)
    else:
        x = (rng.standard_normal((n_rows, ld_x)) * 10.0 ** rng.uniform(-3, 3, (1, ld_x))).astype(np.float32)
    if counted is None:
        rows = None
    elif isinstance(counted, str):
        rows = np.arange(n_rows, dtype=np.int32)
    else:
        rows = np.sort(rng.choice(n_rows, size=counted, replace=False)).astype(np.int32)
    use = np.arange(n_rows) if rows is None else rows
    x[:, n:] = np.nan                                    # padding columns and uncounted rows are never read
    x[np.setdiff1d(np.arange(n_rows), use)] = np.nan
    if start == "zero":
        s0, g0 = np.zeros(n), np.zeros((n, n))
    elif start == "lattice":
        s0, g0 = rng.integers(-99, 100, n).astype(np.float64), rng.integers(-99, 100, (n, n)).astype(np.float64)
    else:
        s0, g0 = rng.standard_normal(n), rng.standard_normal((n, n))
    g0 = np.triu(g0) + np.triu(g0, 1).T                  # a table of the kernel's own making is symmetric
    g = np.full((n, ld_gram), -7.25)                     # the sentinel of the columns >= n
    g[:, :n] = g0
    return x, rows, use, s0, g


def reference(x, use, n, s0, g0, slabs):
    """-> (exact sums and Gram as long double, the bound per element of each)"""
    xs = x[use][:, :n].astype(np.longdouble)
    S, C = xs.sum(0) + s0, xs.T @ xs + g0
    u = 2.0 ** -53
    m = len(use) + slabs + 1
    gam = m * u / (1 - m * u)
    return S, C, gam * (np.abs(s0) + np.abs(xs).sum(0)), gam * (np.abs(g0) + np.abs(xs).T @ np.abs(xs))


def run(shapes, sanitize=False, cxx="g++", verbose=True) -> int:
    bad = 0
    rng = np.random.default_rng(26)
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "gram_host.cpp"), os.path.join(d, "gram_host")
        open(src, "w").write(host_source())
        subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", *(["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []),
                        "-o", exe, src], check=True)
        for n_rows, ld_x, n, counted, ld_gram, slabs, data, start in shapes:
            x, rows, use, s0, g = make_case(rng, n_rows, ld_x, n, counted, ld_gram, data, start)
            nx, ng = (n_rows - 1) * ld_x + n, (n - 1) * ld_gram + n
            fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
            with open(fin, "wb") as f:
                f.write(np.array([n_rows, ld_x, n, -1 if rows is None else len(rows), ld_gram, slabs], np.int32).tobytes() + x.ravel()[:nx].tobytes()
                        + (b"" if rows is None else rows.tobytes()) + s0.tobytes() + g.ravel()[:ng].tobytes())
            res = subprocess.run([exe, fin, fout], check=True, capture_output=True, text=True)
            out = np.fromfile(fout, np.float64)
            got_s, flat = out[:n], np.full(n * ld_gram, -7.25)
            flat[:ng] = out[n:]
            got = flat.reshape(n, ld_gram)
            used = int(res.stdout.split()[1])   # the program's first line: "slabs <how many it ran with>"
            S, C, bs, bc = reference(x, use, n, s0, g[:, :n], used)
            if data == "lattice" and start != "real":
                values = bool((got_s == S.astype(np.float64)).all() and (got[:, :n] == C.astype(np.float64)).all())
            else:
                values = bool((np.abs(got_s - S) <= bs).all() and (np.abs(got[:, :n] - C) <= bc).all())
            ok = [values, bool((got[:, :n].view(np.uint64) == np.ascontiguousarray(got[:, :n].T).view(np.uint64)).all()), bool((got[:, n:] == -7.25).all())]
            bad += not all(ok)
            if verbose:
                print(f"rows {n_rows:3d} ld_x {ld_x:3d} n {n:3d} counted {len(use):3d} slabs {used:3d} {data:7s} values {'ok' if ok[0] else 'DIFFER'}"
                      f"  mirror {'ok' if ok[1] else 'DIFFERS'}  columns >= n {'ok' if ok[2] else 'TOUCHED'}")
        if verbose:
            print(res.stdout, end="")
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
