#!/usr/bin/env python3
"""The PCA kernels' core on the CPU: compiles the text between the PCA-CORE marks of csrc/spv_pca.h -- the slab plan and the workspace
layout, the staging maps, the lane -> operand and lane -> result maps of the fp32 MFMA, the guarded source address, the operand
function (weight, log1p, centre, scale) and the merge, exactly as the kernels use them -- as plain C++, with a driver that walks the
grids the way pca_stage_kernel / pca_project_kernel / pca_back_kernel / pca_merge_kernel do: 256 emulated threads per workgroup, 64
emulated lanes per wave and a chain of fmaf in place of v_mfma_f32_32x32x2_f32 (A[i][k] from lane 32 k + i, B[k][j] from lane 32 k + j, k
ascending).  The results are then compared with numpy:

  * the staged block must EQUAL a numpy fp32 model of the operand bit for bit (the same operations in the same order: no contraction,
    no library log), hold exactly -mu * scale at every zero count, and lie within ``STAGE_UNITS`` units of 2^-24 max(1, a) of the fp64
    definition with np.log1p (the worst value seen is printed);
  * project and back must lie within the elementwise classical bound of the fp64 products of the dumped block: (K + 2) 2^-24 sum |x||v|
    with K the contraction length (G, or the slab length), plus n_slabs 2^-53 |Z| for the fp64 merge;
  * the list in one piece and in slab-aligned pieces must agree bit for bit, a row of project must not depend on the other rows, and
    rows outside the matrix must read as zero counts; padding of the matrix, columns >= l and rows that are not listed hold NaN or a
    sentinel that must never arrive anywhere.
No GPU, nothing loaded into Python.  It checks everything except the MFMA instruction itself.

    python tools/pca_host_check.py [--cxx g++] [--small]"""
import argparse
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np

STAGE_UNITS = 4.0   # units of 2^-24 max(1, a) this tool allows the log1p over its sweep (worst seen 1.86; tests/test_zz_gpu_pca.py holds its own inputs to 3.82)

SHIMS = """#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#define __host__
#define __device__
#define __forceinline__ inline
"""
MAIN = r"""
struct Args {
  const void* X; long ld; const int* rows; int col_off; int u16;
  int G, n_rows, n_piece, pos_off, n, l;
  const float* w; const float* mu; const float* scale;
  float* block; long ld_block; const float* V; long ld_v; float* Y; long ld_y; double* Z; long ld_z; float* ws;
};
static float count_at(const Args& a, long at) { return a.u16 ? (float)((const unsigned short*)a.X)[at] : ((const float*)a.X)[at]; }

// the MFMA's stand-in over the 64 lanes of a wave: D = A B + C, A[i][k] in lane 32 k + i, B[k][j] in lane 32 k + j, a chain of fmaf in k
static void mfma_32x32x2(const float* av, const float* bv, float (*acc)[16]) {
  for (int lane = 0; lane < 64; ++lane)
    for (int reg = 0; reg < 16; ++reg) {
      const int i = pca_result_row(lane, reg), j = pca_result_col(lane);
      float s = acc[lane][reg];
      for (int k = 0; k < 2; ++k) s = fmaf(av[32 * k + i], bv[32 * k + j], s);
      acc[lane][reg] = s;
    }
}

static void stage(const Args& a) {
  const int p_end = a.pos_off + a.n_piece;
  for (int bx = 0; bx < (a.n_piece + PCA_ST_P - 1) / PCA_ST_P; ++bx)
    for (int by = 0; by < (a.G + PCA_THREADS - 1) / PCA_THREADS; ++by)
      for (int t = 0; t < PCA_THREADS; ++t) {
        const int j = by * PCA_THREADS + t;
        const bool g_ok = j < a.G;
        const float mu = (a.mu && g_ok) ? a.mu[j] : 0.f, sc = (a.scale && g_ok) ? a.scale[j] : 1.f;
        for (int i = 0; i < PCA_ST_P; ++i) {
          const int p = a.pos_off + bx * PCA_ST_P + i, q = pca_position(p, p_end);
          const int r = a.rows ? a.rows[q - a.pos_off] : q - a.pos_off;
          const bool ok = g_ok && r >= 0 && r < a.n_rows;
          const float c = count_at(a, pca_source(ok, r, a.ld, a.col_off, j));
          const float wv = a.w ? a.w[q] : 1.f;
          if (p < p_end && g_ok) a.block[(long)(p - a.pos_off) * a.ld_block + j] = pca_operand(ok ? c : 0.f, wv, a.w != nullptr, mu, sc);
        }
      }
}

static void project(const Args& a) {
  const int p_end = a.pos_off + a.n_piece;
  std::vector<float> xs(PCA_KT * PCA_LDX), vs(PCA_KT * PCA_LDV);
  for (int bx = 0; bx < (a.n_piece + PCA_CELL_TILE - 1) / PCA_CELL_TILE; ++bx) {
    const int p0 = a.pos_off + bx * PCA_CELL_TILE;
    static float acc[4][64][16];
    memset(acc, 0, sizeof(acc));
    for (int kt = 0; kt < (a.G + PCA_KT - 1) / PCA_KT; ++kt) {
      const int j0 = kt * PCA_KT;
      for (size_t e = 0; e < xs.size(); ++e) xs[e] = NAN;
      for (size_t e = 0; e < vs.size(); ++e) vs[e] = NAN;
      for (int t = 0; t < PCA_THREADS; ++t) {
        const int gl = pca_pj_gene(t), j = j0 + gl, vc = pca_col(t);
        const bool g_ok = j < a.G;
        const float mu = (a.mu && g_ok) ? a.mu[j] : 0.f, sc = (a.scale && g_ok) ? a.scale[j] : 1.f;
        for (int m = 0; m < 8; ++m) {
          const int q = pca_position(p0 + pca_pj_cell(t, m), p_end);
          const int r = a.rows ? a.rows[q - a.pos_off] : q - a.pos_off;
          const bool r_ok = r >= 0 && r < a.n_rows;
          const float c = count_at(a, pca_source(g_ok && r_ok, r, a.ld, a.col_off, j));
          xs[gl * PCA_LDX + pca_pj_cell(t, m)] = g_ok ? pca_operand(r_ok ? c : 0.f, a.w ? a.w[q] : 1.f, a.w != nullptr, mu, sc) : 0.f;
          const int k = pca_k4(t, m), jv = j0 + k;
          vs[k * PCA_LDV + vc] = (vc < a.l && jv < a.G) ? a.V[(long)jv * a.ld_v + vc] : 0.f;
        }
      }
      for (int wave = 0; wave < 4; ++wave) {
        const int rb = pca_wave_lo(wave), cb = pca_wave_col(wave);
        if (!(32 * cb < a.l)) continue;
        for (int ks = 0; ks < PCA_KT / 2; ++ks) {
          float av[64], bv[64];
          for (int lane = 0; lane < 64; ++lane) {
            av[lane] = xs[pca_operand_at(lane, ks, 32 * rb, PCA_LDX)];
            bv[lane] = vs[pca_operand_at(lane, ks, 32 * cb, PCA_LDV)];
          }
          mfma_32x32x2(av, bv, acc[wave]);
        }
      }
    }
    for (int wave = 0; wave < 4; ++wave) {
      const int rb = pca_wave_lo(wave), cb = pca_wave_col(wave);
      if (!(32 * cb < a.l)) continue;
      for (int lane = 0; lane < 64; ++lane)
        for (int reg = 0; reg < 16; ++reg) {
          const int p = p0 + 32 * rb + pca_result_row(lane, reg), t = 32 * cb + pca_result_col(lane);
          if (p < p_end && t < a.l) a.Y[(long)p * a.ld_y + t] = acc[wave][lane][reg];
        }
    }
  }
}

static void back(const Args& a) {
  const int p_end = a.pos_off + a.n_piece, Gp = pca_gene_pad(a.G);
  std::vector<float> xs(PCA_KT * PCA_LDV), ys(PCA_KT * PCA_LDV);
  for (int bx = 0; bx < Gp / PCA_GENE_TILE; ++bx)
    for (int slab = 0; slab < pca_slabs(a.n_piece); ++slab) {
      const int g0 = bx * PCA_GENE_TILE, p_lo = a.pos_off + slab * PCA_SLAB, p_hi = p_lo + PCA_SLAB < p_end ? p_lo + PCA_SLAB : p_end;
      static float acc[4][64][16];
      memset(acc, 0, sizeof(acc));
      for (int kt = 0; kt < (p_hi - p_lo + PCA_KT - 1) / PCA_KT; ++kt) {
        const int pt = p_lo + kt * PCA_KT;
        for (size_t e = 0; e < xs.size(); ++e) xs[e] = ys[e] = NAN;
        for (int t = 0; t < PCA_THREADS; ++t) {
          const int j = g0 + pca_col(t), vc = pca_col(t);
          const bool g_ok = j < a.G, vc_ok = vc < a.l;
          const float mu = (a.mu && g_ok) ? a.mu[j] : 0.f, sc = (a.scale && g_ok) ? a.scale[j] : 1.f;
          for (int m = 0; m < 8; ++m) {
            const int k = pca_k4(t, m), p = pt + k, q = pca_position(p, p_hi);
            const int r = a.rows ? a.rows[q - a.pos_off] : q - a.pos_off;
            const bool ok = g_ok && r >= 0 && r < a.n_rows, live = p < p_hi;
            const float c = count_at(a, pca_source(ok, r, a.ld, a.col_off, j));
            const float yv = a.Y[(long)q * a.ld_y + (vc_ok ? vc : 0)];
            xs[k * PCA_LDV + pca_col(t)] = (live && g_ok) ? pca_operand(ok ? c : 0.f, a.w ? a.w[q] : 1.f, a.w != nullptr, mu, sc) : 0.f;
            ys[k * PCA_LDV + vc] = (live && vc_ok) ? yv : 0.f;
          }
        }
        for (int wave = 0; wave < 4; ++wave) {
          const int gb = pca_wave_lo(wave), cb = pca_wave_col(wave);
          if (!(32 * cb < a.l)) continue;
          for (int ks = 0; ks < PCA_KT / 2; ++ks) {
            float av[64], bv[64];
            for (int lane = 0; lane < 64; ++lane) {
              av[lane] = xs[pca_operand_at(lane, ks, 32 * gb, PCA_LDV)];
              bv[lane] = ys[pca_operand_at(lane, ks, 32 * cb, PCA_LDV)];
            }
            mfma_32x32x2(av, bv, acc[wave]);
          }
        }
      }
      for (int wave = 0; wave < 4; ++wave) {
        const int gb = pca_wave_lo(wave), cb = pca_wave_col(wave);
        if (!(32 * cb < a.l)) continue;
        for (int lane = 0; lane < 64; ++lane)
          for (int reg = 0; reg < 16; ++reg) {
            const int gene = g0 + 32 * gb + pca_result_row(lane, reg), t = 32 * cb + pca_result_col(lane);
            if (t < a.l) a.ws[pca_ws_at(slab, Gp, gene, a.l, t)] = acc[wave][lane][reg];
          }
      }
    }
  for (long e = 0; e < (long)a.G * a.l; ++e) {   // pca_merge_kernel
    const int j = (int)(e / a.l), t = (int)(e % a.l);
    double* const z = a.Z + (long)j * a.ld_z + t;
    *z = pca_merge(*z, a.ws + pca_ws_at(0, Gp, j, a.l, t), (long)Gp * a.l, pca_slabs(a.n_piece));
  }
}

template <typename T>
static std::vector<T> slurp(FILE* f, size_t count) {
  std::vector<T> v(count);
  if (count && fread(v.data(), sizeof(T), count, f) != count) { fprintf(stderr, "short input\n"); exit(2); }
  return v;
}

// in: header int32 [12] = n, G, n_rows, ld, col_off, u16, l, has_rows, has_w, has_mu, has_scale, piece; then X, rows, w, mu, scale, V, Z
// out: block [n][G], Y [n][l], Z [G][l]
int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "shapes")) {
    printf("%d %d %lld %lld %lld %lld\n", PCA_SLAB, PCA_CELL_TILE, pca_ws_bytes(200, 70, 16), pca_ws_bytes(10000, 4096, 64), pca_ws_bytes(97, 2085, 48),
           pca_ws_bytes(97, 2085, 40));
    return 0;
  }
  FILE* f = fopen(argv[1], "rb");
  const std::vector<int> h = slurp<int>(f, 12);
  const int n = h[0], G = h[1], n_rows = h[2], ld = h[3], col_off = h[4], u16 = h[5], l = h[6], piece = h[11];
  const std::vector<unsigned char> X = slurp<unsigned char>(f, (size_t)n_rows * ld * (u16 ? 2 : 4));
  const std::vector<int> rows = slurp<int>(f, h[7] ? n : 0);
  const std::vector<float> w = slurp<float>(f, h[8] ? n : 0), mu = slurp<float>(f, h[9] ? G : 0), scale = slurp<float>(f, h[10] ? G : 0);
  const std::vector<float> V = slurp<float>(f, (size_t)G * l);
  std::vector<double> Z = slurp<double>(f, (size_t)G * l);
  fclose(f);
  std::vector<float> block((size_t)n * G, -777.f), Y((size_t)n * l, -777.f);
  Args a{X.data(), ld, nullptr, col_off, u16, G, n_rows, 0, 0, n, l, h[8] ? w.data() : nullptr, h[9] ? mu.data() : nullptr, h[10] ? scale.data() : nullptr,
         nullptr, G, V.data(), l, Y.data(), l, Z.data(), l, nullptr};
  const int step = piece > 0 ? piece : n;
  if (step % PCA_SLAB && step < n) { fprintf(stderr, "piece off a slab bound\n"); return 2; }
  for (int p0 = 0; p0 < n; p0 += step) {
    a.pos_off = p0, a.n_piece = p0 + step < n ? step : n - p0;
    a.rows = h[7] ? rows.data() + p0 : nullptr;
    if (!h[7] && p0) { fprintf(stderr, "pieces need a row list\n"); return 2; }
    a.block = block.data() + (size_t)p0 * G;
    std::vector<float> ws((size_t)pca_ws_floats(G, a.n_piece, l), NAN);   // exactly the stated size
    a.ws = ws.data();
    stage(a);
    project(a);
    back(a);
  }
  FILE* o = fopen(argv[2], "wb");
  fwrite(block.data(), 4, block.size(), o);
  fwrite(Y.data(), 4, Y.size(), o);
  fwrite(Z.data(), 8, Z.size(), o);
  fclose(o);
  return 0;
}
"""


def core_text() -> str:
    text = open(os.path.join(ROOT, "spvipes_amd", "csrc", "spv_pca.h")).read()
    return text[text.index("// ---- PCA-CORE-BEGIN ----"):text.index("// ---- PCA-CORE-END ----")]


def build(cxx: str, tmp: str) -> str:
    src, exe = os.path.join(tmp, "pca_core.cpp"), os.path.join(tmp, "pca_core")
    with open(src, "w") as f:
        f.write(SHIMS + core_text() + MAIN)
    subprocess.run([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-Wno-unknown-pragmas", "-o", exe, src], check=True)
    return exe


F = np.float32


def log1p_model(u: np.ndarray) -> np.ndarray:
    """pca_log1p in numpy fp32, operation by operation"""
    u = u.astype(F)
    pos = u > 0
    v = np.where(pos, u, F(1)).astype(F)
    t = (F(1) + v).astype(F)
    c = np.where(v < 1, v - (t - F(1)), F(1) - (t - v)).astype(F)
    m, e = np.frexp(t)
    low = m < F(0.70710678)
    m = np.where(low, m + m, m).astype(F)
    e = np.where(low, e - 1, e)
    f = (m - F(1)).astype(F)
    s = (f / (F(2) + f)).astype(F)
    z = (s * s).astype(F)
    w = (z * z).astype(F)
    t1 = (w * (F(0.40000972152) + (w * F(0.24279078841)).astype(F)).astype(F)).astype(F)
    t2 = (z * (F(0.66666662693) + (w * F(0.28498786688)).astype(F)).astype(F)).astype(F)
    r = (t2 + t1).astype(F)
    hfsq = ((F(0.5) * f).astype(F) * f).astype(F)
    dk = e.astype(F)
    inner = ((s * (hfsq + r).astype(F)).astype(F) + (dk * F(9.0580006145e-06)).astype(F)).astype(F)
    lg = ((dk * F(6.9313812256e-01)).astype(F) - ((hfsq - inner).astype(F) - f).astype(F)).astype(F)
    return np.where(pos, (lg + (c / t).astype(F)).astype(F), F(0)).astype(F)


def operand_model(c, w, mu, scale) -> np.ndarray:
    """x(p, j) in numpy fp32: c [n, G] counts as fp32, w [n] or None, mu / scale [G] or None"""
    u = c.astype(F) if w is None else (c.astype(F) * w.astype(F)[:, None]).astype(F)
    a = log1p_model(u)
    d = a if mu is None else (a - mu.astype(F)[None, :]).astype(F)
    return d if scale is None else (d * scale.astype(F)[None, :]).astype(F)


def run_case(exe, tmp, name, n, G, l, dtype, col_off, with_rows, with_w, with_mu, with_scale, piece, seed, bad_row=False, z_start=False):
    rng = np.random.default_rng(seed)
    n_rows, ld = n + 9, col_off + G + 3
    dens = rng.random((n_rows, G)) < 0.25
    counts = (rng.poisson(3.0, (n_rows, G)) * dens).astype(np.float64)
    counts[1, :] = 0                                                   # a cell without counts
    if dtype == "u16":
        counts[2, G // 2] = 65535
        X = np.full((n_rows, ld), 0xFFFF, np.uint16)                   # padding that must not be read as data
        X[:, col_off:col_off + G] = counts.astype(np.uint16)
    else:
        counts = counts * 1.5
        X = np.full((n_rows, ld), np.nan, np.float32)
        X[:, col_off:col_off + G] = counts.astype(np.float32)
    rows = None
    if with_rows:
        rows = rng.permutation(n_rows)[:n].astype(np.int32)
        rows[:3] = [1, 2, 0]
        if bad_row:
            rows[5], rows[6] = -4, n_rows + 2                         # outside the matrix: zero counts, never read
    src = np.arange(n) if rows is None else rows
    ok = (src >= 0) & (src < n_rows)
    c = np.where(ok[:, None], counts[np.clip(src, 0, n_rows - 1)], 0.0)
    w = None
    if with_w:
        tot = c.sum(1)
        w = np.where(tot > 0, 1e4 / np.maximum(tot, 1), 0).astype(F)
    mu = rng.random(G).astype(F) if with_mu else None
    scale = None
    if with_scale:
        scale = (0.5 + rng.random(G)).astype(F)
        scale[rng.random(G) < 0.2] = 0
    V = rng.standard_normal((G, l)).astype(F)
    Z0 = rng.standard_normal((G, l)) if z_start else np.zeros((G, l))
    path_in, path_out = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(path_in, "wb") as f:
        f.write(np.array([n, G, n_rows, ld, col_off, dtype == "u16", l, with_rows, with_w, with_mu, with_scale, piece], np.int32).tobytes())
        f.write(X.tobytes())
        for arr in (rows, w, mu, scale):
            if arr is not None:
                f.write(arr.tobytes())
        f.write(V.tobytes())
        f.write(Z0.astype(np.float64).tobytes())
    subprocess.run([exe, path_in, path_out], check=True)
    raw = open(path_out, "rb").read()
    block = np.frombuffer(raw, F, n * G).reshape(n, G)
    Y = np.frombuffer(raw, F, n * l, offset=4 * n * G).reshape(n, l)
    Z = np.frombuffer(raw, np.float64, G * l, offset=4 * n * (G + l)).reshape(G, l)
    # the operand: bit for bit against the fp32 model, zero counts exactly -mu * scale, and close to the fp64 definition
    model = operand_model(c.astype(F), w, mu, scale)
    assert np.array_equal(block.view(np.uint32), model.view(np.uint32)), f"{name}: the staged block differs from the fp32 model"
    zero = c == 0
    expect0 = np.broadcast_to(((F(0) - (mu if mu is not None else np.zeros(G, F))) * (scale if scale is not None else np.ones(G, F))).astype(F)[None, :], block.shape)
    assert np.array_equal(block[zero].view(np.uint32), expect0[zero].view(np.uint32)), f"{name}: a zero count is not -mu * scale"
    u64 = c.astype(F).astype(np.float64) if w is None else (c.astype(F) * w[:, None]).astype(F).astype(np.float64)
    a64 = np.log1p(u64)
    a32 = log1p_model(u64.astype(F)).astype(np.float64)
    units = float(np.max(np.abs(a32 - a64) / (2.0 ** -24 * np.maximum(1.0, a64))))
    assert units <= STAGE_UNITS, f"{name}: log1p is {units} units of 2^-24 max(1, a) off"
    # project and back against fp64 products of the dumped block
    b64 = block.astype(np.float64)
    Yref, Ybound = b64 @ V.astype(np.float64), (G + 2) * 2.0 ** -24 * (np.abs(b64) @ np.abs(V.astype(np.float64)))
    assert np.all(np.abs(Y - Yref) <= Ybound), f"{name}: project outside the bound"
    y64 = Y.astype(np.float64)
    slab = 1024
    n_slabs = (n + slab - 1) // slab
    Zref = Z0 + b64.T @ y64
    Zbound = (min(slab, n) + 2) * 2.0 ** -24 * (np.abs(b64).T @ np.abs(y64)) + n_slabs * 2.0 ** -53 * (np.abs(Z0) + np.abs(b64).T @ np.abs(y64))
    assert np.all(np.abs(Z - Zref) <= Zbound), f"{name}: back outside the bound"
    used = float(np.max(np.abs(Y - Yref) / np.maximum(Ybound, 1e-300)))
    print(f"  {name}: n {n} G {G} l {l} {dtype} piece {piece or n}: log1p {units:.2f} units, project uses {used:.3f} of its bound")
    return block, Y, Z, units


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--cxx", default="g++")
    ap.add_argument("--small", action="store_true")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(args.cxx, tmp)
        shapes = [int(v) for v in subprocess.run([exe, "shapes"], check=True, capture_output=True, text=True).stdout.split()]
        assert shapes == [1024, 64, 4 * 1 * 256 * 16, 4 * 4 * 10048 * 64, 4 * 3 * 128 * 48, 0], shapes
        assert 4096 % shapes[0] == 0
        # log1p over a sweep of magnitudes, against fp64
        u = np.concatenate([np.logspace(-30, 9, 200001), np.arange(0, 70000, dtype=np.float64), [0.0]]).astype(F)
        a = log1p_model(u).astype(np.float64)
        ref = np.log1p(u.astype(np.float64))
        sweep = float(np.max(np.abs(a - ref) / (2.0 ** -24 * np.maximum(1.0, ref))))
        assert sweep <= STAGE_UNITS and a[-1] == 0.0, sweep
        print(f"  log1p sweep: worst {sweep:.2f} units of 2^-24 max(1, a)")
        worst = sweep
        cases = [("u16-rows-w", 70, 97, 16, "u16", 5, True, True, True, True, 0, 1),
                 ("f32-plain", 70, 200, 48, "f32", 0, False, False, False, False, 0, 2),
                 ("u16-bad-rows", 131, 230, 32, "u16", 0, True, True, True, False, 0, 3)]
        if not args.small:
            cases += [("three-slabs", 2 * 1024 + 37, 97, 64, "u16", 3, True, True, True, True, 0, 4)]
        for name, n, G, l, dtype, col_off, wr, ww, wm, ws_, piece, seed in cases:
            worst = max(worst, run_case(exe, tmp, name, n, G, l, dtype, col_off, wr, ww, wm, ws_, piece, seed, bad_row=name == "u16-bad-rows", z_start=True)[3])
        if not args.small:   # pieces against one piece: the same bits everywhere
            one = run_case(exe, tmp, "three-slabs", 2 * 1024 + 37, 97, 64, "u16", 3, True, True, True, True, 0, 4, z_start=True)
            for piece in (1024, 2048):
                many = run_case(exe, tmp, f"pieces-{piece}", 2 * 1024 + 37, 97, 64, "u16", 3, True, True, True, True, piece, 4, z_start=True)
                for x, y, what in zip(one[:3], many[:3], ("block", "Y", "Z")):
                    assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), f"pieces of {piece}: {what} differs from one piece"
        print(f"pca_host_check: ok (log1p worst {worst:.2f} units)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
