#!/usr/bin/env python3
"""The transport-projection core on the CPU: compiles the text between the OTPROJ-CORE marks of csrc/spv_ot_project.h -- the lane's
state, the update per candidate, the merge of the chunks' states, the final quotient, the workspace's rows and the chunk plan --
behind the KNN-CORE text of csrc/spv_knn.h and the OT-CORE text of csrc/spv_ot.h it builds on, as plain C++ with ot_host_check.py's
one-line stand-ins for the intrinsics (built with -ffp-contract=off), runs it over a few shapes the way the kernels do (one state per
(query, chunk, column block) over the chunk's candidates in ascending order, the chunk plan of knn_chunk, the workspace
[chunk][n_v + 2 * blocks][n_q], one merge per (query, column)) and compares with numpy (tests/_ot_project_reference.py):

  * out of one chunk and out through n_split chunks and otproj_merge must lie within ``project_bound`` of the float64 weighted mean,
    NaN exactly where the reference is NaN (queries whose every t is not finite, n_c = 0);
  * L of both routes must EQUAL, bit for bit, the plain ot_update / ot_merge / ot_lse_value route of ot_softmin_kernel at the same
    chunk plan;
  * column 0 of V is all ones: it must come back as exactly 1.0f on both routes;
  * both block widths (16 and 32) must give the same bits: a column's operations do not depend on its block;
  * the quiet-round route (otproj_stays / otproj_stay, taken here whenever one lane's round allows it) and the plain route
    (otproj_update for every candidate) must give the same bits;
  * every slot of the workspace rows in use must have been written (heap blocks of exactly otproj_ws_bytes).
No GPU, nothing loaded into Python.  It checks the arithmetic and the bookkeeping, not the kernels' indexing.

    python tools/ot_project_host_check.py [--cxx g++] [--small]

A plain build.  --small: the first shapes only."""
import argparse
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np

from tools.ot_host_check import SHIMS, make_case

PROJ_SHIMS = "#include <cstring>\nstatic inline float __fdiv_rn(float a, float b) { return a / b; }\n"
MAIN = """
static OtLse lse_scan(const float* t, int c0, int c1) {
  OtLse a;
  ot_lse_init(a);
  for (int c = c0; c < c1; ++c) ot_update(a, t[c]);
  return a;
}
// what a lane of column block z does with its chunk [c0, c1): the block's value rows with zeros past n_v, as the kernel stages them
template <int VB>
static OtProj<VB> scan_plain(const float* t, const float* V, int n_v, int z, int c0, int c1) {
  OtProj<VB> st;
  otproj_init(st);
  float row[VB];
  for (int c = c0; c < c1; ++c) {
    for (int v = 0; v < VB; ++v) row[v] = z * VB + v < n_v ? V[(size_t)c * n_v + z * VB + v] : 0.f;
    otproj_update(st, t[c], row);
  }
  return st;
}
template <int VB>
static OtProj<VB> scan(const float* t, const float* V, int n_v, int z, int c0, int c1) {
  OtProj<VB> st;
  otproj_init(st);
  constexpr int CAND = 4;   // rounds of CAND candidates from the chunk's start on, as pair_scan offers them; rows past the chunk's end: t = -inf, zeros
  float row[CAND][VB], tr[CAND];
  for (int r = c0; r < c1; r += CAND) {
    bool quiet = true;
    for (int u = 0; u < CAND; ++u) {
      const int c = r + u;
      tr[u] = c < c1 ? t[c] : -INFINITY;
      for (int v = 0; v < VB; ++v) row[u][v] = (c < c1 && z * VB + v < n_v) ? V[(size_t)c * n_v + z * VB + v] : 0.f;
      quiet = quiet && otproj_stays(st, tr[u]);
    }
    for (int u = 0; u < CAND; ++u) {
      if (quiet) otproj_stay(st, tr[u], row[u]);   // the kernel's quiet round (there the vote of a whole wave)
      else otproj_update(st, tr[u], row[u]);
    }
  }
  return st;
}

// out1 / L1: one chunk; out2 / L2: n_split chunks through the workspace and the merge, for queries of t rows
template <int VB>
static int run(int n_q, int n_c, int n_v, int n_split, const float* T, const float* V, float* out1, float* L1, float* out2, float* L2) {
  const int rows = otproj_ws_rows(n_v, VB), blocks = (n_v + VB - 1) / VB, per = knn_chunk(n_c, n_split);
  const size_t nW = (size_t)n_split * rows * n_q;
  if (otproj_ws_bytes(n_q, n_v, n_split) < (long long)(n_split > 1 ? nW * 4 : 0)) return 5;
  float* ws = (float*)malloc(n_split > 1 ? otproj_ws_bytes(n_q, n_v, n_split) : 4);
  for (size_t e = 0; e < (n_split > 1 ? nW : 0); ++e) ws[e] = NAN;
  for (int i = 0; i < n_q; ++i) {
    const float* t = T + (size_t)i * n_c;
    for (int z = 0; z < blocks; ++z) {
      const int n_col = n_v - z * VB < VB ? n_v - z * VB : VB;
      const OtProj<VB> one = scan<VB>(t, V, n_v, z, 0, n_c), plain = scan_plain<VB>(t, V, n_v, z, 0, n_c);
      if (memcmp(&one, &plain, sizeof(one))) return 6;   // the quiet rounds changed a bit
      for (int c = 0; c < n_col; ++c) out1[(size_t)(z * VB + c) * n_q + i] = otproj_value(one.acc[c], one.st);
      if (z == 0) L1[i] = ot_lse_value(one.st);
      for (int k = 0; k < n_split && n_split > 1; ++k) {
        const long first = (long)k * per;
        const int c0 = first < n_c ? (int)first : n_c, c1 = first + per < n_c ? (int)(first + per) : n_c;
        const OtProj<VB> st = scan<VB>(t, V, n_v, z, c0, c1);
        float* const w = ws + ((size_t)k * rows + (size_t)z * (VB + 2)) * n_q + i;
        w[0] = st.st.m;
        w[n_q] = st.st.sum;
        for (int c = 0; c < n_col; ++c) w[(size_t)(2 + c) * n_q] = st.acc[c];
      }
    }
    for (int v = 0; v < n_v; ++v) {   // otproj_merge_kernel's lane (i, v)
      if (n_split == 1) { out2[(size_t)v * n_q + i] = out1[(size_t)v * n_q + i]; L2[i] = L1[i]; continue; }
      const int z = v / VB;
      const float* const w = ws + (size_t)z * (VB + 2) * n_q + i;
      const long chunk = (long)rows * n_q, col = (long)(2 + v - z * VB) * n_q;
      OtLse st;
      ot_lse_init(st);
      float acc = 0.f;
      for (int c = 0; c < n_split; ++c) otproj_merge(st, &acc, 1, OtLse{w[c * chunk], w[c * chunk + n_q]}, w + c * chunk + col, 0);
      out2[(size_t)v * n_q + i] = otproj_value(acc, st);
      if (v == 0) L2[i] = ot_lse_value(st);
    }
  }
  int bad = 0;
  for (size_t e = 0; e < (n_split > 1 ? nW : 0); ++e) bad |= ws[e] != ws[e];   // a slot nobody wrote (no state holds a NaN here)
  free(ws);
  return bad ? 4 : 0;
}

int main(int argc, char** argv) {   // argv: input file, output file
  FILE* f = fopen(argv[1], "rb"); FILE* o = fopen(argv[2], "wb");
  if (!f || !o) return 2;
  int h[5]; float s;   // n_q, n_c, D, n_v, n_split; s
  if (fread(h, 4, 5, f) != 5 || fread(&s, 4, 1, f) != 1) return 3;
  const int n_q = h[0], n_c = h[1], D = h[2], n_v = h[3], n_split = h[4];
  std::vector<float> Q((size_t)n_q * D), C((size_t)n_c * D + 1), hv(n_c + 1), V((size_t)n_c * n_v + 1), T((size_t)n_q * n_c + 1);
  if (fread(Q.data(), 4, Q.size(), f) != Q.size() || fread(C.data(), 4, (size_t)n_c * D, f) != (size_t)n_c * D || fread(hv.data(), 4, n_c, f) != (size_t)n_c
      || fread(V.data(), 4, (size_t)n_c * n_v, f) != (size_t)n_c * n_v) return 3;
  for (int i = 0; i < n_q; ++i)
    for (int c = 0; c < n_c; ++c) T[(size_t)i * n_c + c] = ot_t(knn_d2(Q.data() + (size_t)i * D, C.data() + (size_t)c * D, D), s, hv[c]);
  const size_t nO = (size_t)n_v * n_q;
  std::vector<float> flat(n_q);
  const int per = knn_chunk(n_c, n_split);
  for (int i = 0; i < n_q; ++i) {
    OtLse m;
    ot_lse_init(m);
    for (int c = 0; c < n_split; ++c) {
      const long first = (long)c * per;
      const int c0 = first < n_c ? (int)first : n_c, c1 = first + per < n_c ? (int)(first + per) : n_c;
      ot_merge(m, lse_scan(T.data() + (size_t)i * n_c, c0, c1));
    }
    flat[i] = ot_lse_value(m);
  }
  for (int pass = 0; pass < 2; ++pass) {   // block width 32, then 16
    float* out1 = (float*)malloc(4 * nO); float* out2 = (float*)malloc(4 * nO); float* L1 = (float*)malloc(4 * n_q); float* L2 = (float*)malloc(4 * n_q);
    const int rc = pass == 0 ? run<32>(n_q, n_c, n_v, n_split, T.data(), V.data(), out1, L1, out2, L2)
                             : run<16>(n_q, n_c, n_v, n_split, T.data(), V.data(), out1, L1, out2, L2);
    if (rc) return rc;
    fwrite(out1, 4, nO, o); fwrite(out2, 4, nO, o); fwrite(L1, 4, n_q, o); fwrite(L2, 4, n_q, o);
    free(L2); free(L1); free(out2); free(out1);
  }
  fwrite(flat.data(), 4, n_q, o);
  fclose(o); fclose(f); return 0;
}
"""
# (n_q, n_c, D, n_v, n_split, data, s): "edge" puts -inf / nan / +inf among h and huge rows among the candidates (make_case)
SHAPES = [(5, 40, 3, 4, 3, "lattice", 0.5), (4, 30, 1, 17, 5, "lattice", 1.0), (3, 0, 4, 3, 2, "real", 1.0), (6, 70, 25, 33, 7, "edge", 0.4),
          (5, 50, 10, 1, 4, "real", 0.7), (4, 60, 5, 16, 1, "real", 0.7), (9, 300, 35, 67, 5, "real", 0.3), (8, 120, 25, 32, 64, "edge", 2.0),
          (4, 257, 64, 2, 2, "real", 0.05), (12, 500, 10, 9, 1, "lattice", 3.0)]


def host_source() -> str:
    """the three cores as they stand in the headers, between the stand-ins and a main()"""
    def core(name, tag):
        text = open(os.path.join(ROOT, "spvipes_amd", "csrc", name)).read()
        return text[text.index(f"// ---- {tag}-CORE-BEGIN ----"):text.index(f"// ---- {tag}-CORE-END ----")]
    return SHIMS + PROJ_SHIMS + core("spv_knn.h", "KNN") + core("spv_ot.h", "OT") + core("spv_ot_project.h", "OTPROJ") + MAIN


def run(shapes, cxx="g++", verbose=True) -> int:
    from tests._ot_project_reference import project_bound, project_ref
    from tests._ot_reference import t_ref
    bad = 0
    rng = np.random.default_rng(29)
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "otproj_host.cpp"), os.path.join(d, "otproj_host")
        open(src, "w").write(host_source())
        subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe, src], check=True)
        for n_q, n_c, D, n_v, n_split, kind, s in shapes:
            Q, C, h = make_case(rng, n_q, n_c, D, kind)
            V = rng.standard_normal((n_c, n_v)).astype(np.float32)
            V[:, 0] = 1.0
            if kind == "edge" and n_c >= 12:
                V[[1, 3, 5, 6, 8, 9, 10], 1:] = 3e38   # behind the candidates whose t is not finite: never in a sum
            fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
            with open(fin, "wb") as f:
                f.write(np.array([n_q, n_c, D, n_v, n_split], np.int32).tobytes() + np.float32(s).tobytes() + Q.tobytes() + C.tobytes() + h.tobytes()
                        + V.tobytes())
            subprocess.run([exe, fin, fout], check=True)
            rec = np.fromfile(fout, np.float32)
            n_o = n_v * n_q
            passes = []
            for p in range(2):
                b = rec[p * (2 * n_o + 2 * n_q):]
                passes.append((b[:n_o].reshape(n_v, n_q).T, b[n_o:2 * n_o].reshape(n_v, n_q).T, b[2 * n_o:2 * n_o + n_q], b[2 * n_o + n_q:2 * n_o + 2 * n_q]))
            flat = rec[2 * (2 * n_o + 2 * n_q):]
            t = t_ref(Q, C, h, s)
            want, want_L = project_ref(t, V)
            some = np.isfinite(want_L)
            per = -(-n_c // n_split) if n_c else 0
            out1, out2, L1, L2 = passes[0]
            ok = []
            with np.errstate(invalid="ignore"):
                for out, nc, ns in ((out1, n_c, 1), (out2, per, n_split)):
                    ok.append(bool(np.isnan(out[~some]).all() and (np.abs(out[some].astype(np.float64) - want[some]) <= project_bound(t, V, nc, ns)[some]).all()))
            ok.append(np.array_equal(L2.view(np.uint32), flat.view(np.uint32)) and bool(np.isneginf(L1[~some]).all()))
            ok.append(bool((out1[some, 0] == 1.0).all() and (out2[some, 0] == 1.0).all()))
            ok.append(all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(passes[0], passes[1])))
            bad += not all(ok)
            if verbose:
                names = ("one chunk", "split and merge", "L = softmin", "ones exact", "block 16 = block 32")
                print(f"n_q {n_q:3d} n_c {n_c:3d} D {D:2d} n_v {n_v:3d} n_split {n_split:2d} {kind:8s} "
                      + "  ".join(f"{n} {'ok' if v else 'DIFFERS'}" for n, v in zip(names, ok)))
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--cxx", default="g++")
    a = ap.parse_args()
    bad = run(SHAPES[:6] if a.small else SHAPES, a.cxx)
    print("all within bounds" if not bad else f"{bad} shape(s) DIFFER")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
