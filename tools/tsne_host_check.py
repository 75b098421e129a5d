#!/usr/bin/env python3
"""The t-SNE core on the CPU: compiles the text between the TSNE-CORE marks of csrc/spv_tsne.h -- the pair's weight, a lane's running sums,
the merge of the chunks' sums, the chunk plan and the workspace's size, the perplexity calibration, the attractive term, the gradient,
the step and the fixed-order sum of Zrow -- behind the KNN-CORE text of csrc/spv_knn.h it builds on, as plain C++ with one-line stand-ins
for the rounding intrinsics (built with -ffp-contract=off), runs it the way the kernels do and compares with numpy
(tests/_tsne_reference.py):

  * repulsion: one lane per query over the padded vectors (DP = 4), one chunk, and n_split chunks of knn_chunk through the workspace
    [chunk][1 + D][n_q] and tsne_merge; both must lie within ``repulsion_bound`` of the float64 sums, the two routes within
    ``summation_bound`` of each other, and on the exact case (coordinates 0 / 1, D = 1) agree bit for bit; every slot of the workspace
    (a heap block of exactly tsne_ws_bytes) must have been written;
  * affinities: rows sum to 1, the float64 entropy of a row is within 2e-5 of log(perplexity) where the reference converges, beta and P
    agree with the reference's;
  * update: Z, the gradient, kl_row, u and y_out within ``update_ref``'s bounds, the gains equal wherever the reference is sure of a sign.
No GPU, nothing loaded into Python.  It checks the arithmetic and the bookkeeping, not the kernels' indexing.

    python tools/tsne_host_check.py [--cxx g++] [--small]

A plain build.  --small: the first shapes only."""
import argparse
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np

from tools.ot_host_check import SHIMS

TSNE_SHIMS = """#include <cstring>
static inline float __fdiv_rn(float a, float b) { return a / b; }
static inline float __fadd_rn(float a, float b) { return a + b; }
static inline float __fmul_rn(float a, float b) { return a * b; }
"""
MAIN = """
template <typename T> static std::vector<T> rd(FILE* f, size_t n) { std::vector<T> v(n + 1); if (fread(v.data(), sizeof(T), n, f) != n) exit(3); return v; }
static void wr(FILE* o, const double* p, size_t n) { fwrite(p, 8, n, o); }

// a lane's scan of the candidates [c0, c1), `ex` left out: the padded vectors, zeros from D on
static TsneSums scan(const float* q4, const float* C4, int c0, int c1, int ex) {
  TsneSums s;
  tsne_sums_init(s);
  for (int j = c0; j < c1; ++j)
    if (j != ex) tsne_add(s, q4, C4 + (size_t)j * TSNE_DMAX, knn_d2(q4, C4 + (size_t)j * TSNE_DMAX, TSNE_DMAX));
  return s;
}

static int repulsion(FILE* f, FILE* o) {
  const std::vector<int> h = rd<int>(f, 5);
  const int n_q = h[0], n_c = h[1], D = h[2], n_split = h[3], use_ex = h[4];
  const std::vector<float> Q = rd<float>(f, (size_t)n_q * D), C = rd<float>(f, (size_t)n_c * D);
  const std::vector<int> ex = rd<int>(f, n_q);
  std::vector<float> Q4((size_t)n_q * 4, 0.f), C4((size_t)n_c * 4 + 4, 0.f);
  for (int i = 0; i < n_q; ++i) for (int t = 0; t < D; ++t) Q4[(size_t)i * 4 + t] = Q[(size_t)i * D + t];
  for (int j = 0; j < n_c; ++j) for (int t = 0; t < D; ++t) C4[(size_t)j * 4 + t] = C[(size_t)j * D + t];
  std::vector<double> Z1(n_q), F1((size_t)D * n_q), Z2(n_q), F2((size_t)D * n_q);
  const int per = knn_chunk(n_c, n_split);
  const size_t nW = (size_t)n_split * (1 + D) * n_q;
  if (tsne_ws_bytes(n_q, D, n_split) != (long long)(n_split > 1 ? nW * 8 : 0)) return 5;
  double* ws = (double*)malloc(n_split > 1 ? nW * 8 : 8);
  for (size_t e = 0; e < (n_split > 1 ? nW : 0); ++e) ws[e] = NAN;
  for (int i = 0; i < n_q; ++i) {
    const int e = use_ex ? ex[i] : -1;
    const TsneSums one = scan(Q4.data() + (size_t)i * 4, C4.data(), 0, n_c, e);
    Z1[i] = one.z;
    for (int t = 0; t < D; ++t) F1[(size_t)t * n_q + i] = one.f[t];
    for (int t = D; t < TSNE_DMAX; ++t) if (one.f[t] != 0.0) return 6;   // a padded dimension gathered something
    if (n_split == 1) { Z2[i] = Z1[i]; for (int t = 0; t < D; ++t) F2[(size_t)t * n_q + i] = F1[(size_t)t * n_q + i]; continue; }
    for (int k = 0; k < n_split; ++k) {
      const long first = (long)k * per;
      const int c0 = first < n_c ? (int)first : n_c, c1 = first + per < n_c ? (int)(first + per) : n_c;
      const TsneSums s = scan(Q4.data() + (size_t)i * 4, C4.data(), c0, c1, e);
      double* const out = ws + (size_t)k * (1 + D) * n_q + i;
      out[0] = s.z;
      for (int t = 0; t < D; ++t) out[(size_t)(1 + t) * n_q] = s.f[t];
    }
    Z2[i] = tsne_merge(ws + i, (long)(1 + D) * n_q, n_split);
    for (int t = 0; t < D; ++t) F2[(size_t)t * n_q + i] = tsne_merge(ws + (size_t)(1 + t) * n_q + i, (long)(1 + D) * n_q, n_split);
  }
  int bad = 0;
  for (size_t e = 0; e < (n_split > 1 ? nW : 0); ++e) bad |= ws[e] != ws[e];
  free(ws);
  if (bad) return 4;
  wr(o, Z1.data(), n_q); wr(o, F1.data(), F1.size()); wr(o, Z2.data(), n_q); wr(o, F2.data(), F2.size());
  return 0;
}

static int affinities(FILE* f, FILE* o) {
  const std::vector<int> h = rd<int>(f, 2);
  const int n = h[0], k = h[1];
  const std::vector<double> perp = rd<double>(f, 1);
  const std::vector<float> d2 = rd<float>(f, (size_t)n * k);
  std::vector<float> P((size_t)n * k);
  std::vector<double> beta(n), P64((size_t)n * k);
  for (int i = 0; i < n; ++i) beta[i] = tsne_calibrate(d2.data() + (size_t)i * k, k, log(perp[0]), P.data() + (size_t)i * k);
  for (size_t e = 0; e < P.size(); ++e) P64[e] = P[e];
  wr(o, P64.data(), P64.size()); wr(o, beta.data(), n);
  return 0;
}

static int update(FILE* f, FILE* o) {
  const std::vector<int> h = rd<int>(f, 3);
  const int n = h[0], D = h[1], nnz = h[2];
  const std::vector<double> par = rd<double>(f, 4);   // alpha, momentum, lr, min_gain
  const std::vector<long> indptr = rd<long>(f, n + 1);
  const std::vector<int> cols = rd<int>(f, nnz);
  const std::vector<float> vals = rd<float>(f, nnz), y = rd<float>(f, (size_t)n * D);
  std::vector<float> u = rd<float>(f, (size_t)n * D), gain = rd<float>(f, (size_t)n * D);
  const std::vector<double> Zrow = rd<double>(f, n), F = rd<double>(f, (size_t)D * n);
  double part[TSNE_ZSUM_T];
  for (int l = 0; l < TSNE_ZSUM_T; ++l) part[l] = tsne_zsum_lane(Zrow.data(), n, l);
  for (int hh = TSNE_ZSUM_T / 2; hh >= 1; hh /= 2)
    for (int l = 0; l < hh; ++l) tsne_zsum_fold(part, l, hh);
  const double Z = part[0];
  std::vector<double> grad((size_t)D * n), kl(n), g64((size_t)n * D), u64((size_t)n * D), y64((size_t)n * D);
  for (int i = 0; i < n; ++i) {
    double A[TSNE_DMAX];
    tsne_attract(y.data(), D, n, D, i, cols.data(), vals.data(), indptr[i], indptr[i + 1], A, kl[i]);
    for (int t = 0; t < D; ++t) {
      const double g = tsne_grad(par[0], A[t], F[(size_t)t * n + i], Z);
      grad[(size_t)t * n + i] = g;
      y64[(size_t)i * D + t] = tsne_step(y[(size_t)i * D + t], u[(size_t)i * D + t], gain[(size_t)i * D + t], g, par[1], par[2], par[3]);
      u64[(size_t)i * D + t] = u[(size_t)i * D + t];
      g64[(size_t)i * D + t] = gain[(size_t)i * D + t];
    }
  }
  wr(o, &Z, 1); wr(o, grad.data(), grad.size()); wr(o, kl.data(), n); wr(o, g64.data(), g64.size()); wr(o, u64.data(), u64.size()); wr(o, y64.data(), y64.size());
  return 0;
}

int main(int argc, char** argv) {   // argv: input file, output file
  FILE* f = fopen(argv[1], "rb"); FILE* o = fopen(argv[2], "wb");
  if (!f || !o) return 2;
  int mode;
  if (fread(&mode, 4, 1, f) != 1) return 3;
  const int rc = mode == 0 ? repulsion(f, o) : mode == 1 ? affinities(f, o) : update(f, o);
  fclose(o); fclose(f); return rc;
}
"""
# (kind, n_q, n_c, D, n_split, exclude)
SHAPES = [("spread", 5, 40, 2, 3, False), ("same", 30, 30, 3, 5, True), ("spread", 3, 0, 4, 2, False), ("dups", 6, 70, 1, 7, False),
          ("far", 8, 64, 2, 1, False), ("exact", 9, 130, 1, 4, False), ("spread", 40, 300, 4, 5, False), ("same", 129, 257, 2, 64, True),
          ("far", 12, 500, 3, 2, False), ("exact", 33, 1000, 1, 13, False)]
AFFINITIES = [(30, 12, 4.0), (60, 64, 20.0), (25, 60, 30.0)]


def host_source() -> str:
    """the two cores as they stand in the headers, between the stand-ins and a main()"""
    def core(name, tag):
        text = open(os.path.join(ROOT, "spvipes_amd", "csrc", name)).read()
        return text[text.index(f"// ---- {tag}-CORE-BEGIN ----"):text.index(f"// ---- {tag}-CORE-END ----")]
    return SHIMS + TSNE_SHIMS + core("spv_knn.h", "KNN") + core("spv_tsne.h", "TSNE") + MAIN


def affinity_rows(rng, n: int, k: int):
    """ascending squared distances with rows of every kind: ordinary, some empty slots, all equal, all empty"""
    d2 = np.sort(rng.gamma(2.0, 2.0, (n, k)).astype(np.float32), axis=1)
    d2[1, k // 2:] = np.inf
    d2[2, :] = 1.5
    d2[3, :] = np.inf
    d2[4, 1:] = np.inf
    return d2


def run(shapes, affs, cxx="g++", verbose=True) -> int:
    from tests import _tsne_reference as R
    bad = 0
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "tsne_host.cpp"), os.path.join(d, "tsne_host")
        open(src, "w").write(host_source())
        subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe, src], check=True)
        fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")

        def call(blob):
            open(fin, "wb").write(blob)
            subprocess.run([exe, fin, fout], check=True)
            return np.fromfile(fout, np.float64)

        for kind, n_q, n_c, D, n_split, use_ex in shapes:
            Q, C = R.exact_case(n_q, n_c) if kind == "exact" else R.repulsion_case(kind, n_q, n_c, D)
            ex = np.arange(n_q, dtype=np.int32)
            rec = call(np.array([0, n_q, n_c, D, n_split, int(use_ex)], np.int32).tobytes() + Q.tobytes() + C.tobytes() + ex.tobytes())
            Z1, F1, Z2, F2 = rec[:n_q], rec[n_q:n_q * (1 + D)].reshape(D, n_q), rec[n_q * (1 + D):n_q * (2 + D)], rec[n_q * (2 + D):].reshape(D, n_q)
            ref = R.repulsion_ref(Q, C, ex if use_ex else None)
            bZ, bF = R.repulsion_bound(ref, D)
            sZ, sF = R.summation_bound(ref)
            ok = [bool((np.abs(Z1 - ref["Z"]) <= bZ).all() and (np.abs(F1 - ref["F"]) <= bF).all()),
                  bool((np.abs(Z2 - ref["Z"]) <= bZ).all() and (np.abs(F2 - ref["F"]) <= bF).all()),
                  bool((np.abs(Z1 - Z2) <= sZ).all() and (np.abs(F1 - F2) <= sF).all()),
                  kind != "exact" or (np.array_equal(Z1, Z2) and np.array_equal(F1, F2) and np.array_equal(Z1, ref["Z"]) and np.array_equal(F1, ref["F"]))]
            bad += not all(ok)
            if verbose:
                names = ("one chunk", "split and merge", "routes agree", "exact case bit for bit")
                print(f"repulsion {kind:7s} n_q {n_q:3d} n_c {n_c:4d} D {D} n_split {n_split:2d} "
                      + "  ".join(f"{n} {'ok' if v else 'DIFFERS'}" for n, v in zip(names, ok)))
        rng = np.random.default_rng(31)
        for n, k, perp in affs:
            d2 = affinity_rows(rng, n, k)
            rec = call(np.array([1, n, k], np.int32).tobytes() + np.float64(perp).tobytes() + d2.tobytes())
            P, beta = rec[:n * k].reshape(n, k), rec[n * k:]
            Pr, br, conv = R.affinities_ref(d2, perp)
            some = np.isfinite(d2[:, 0])
            H = np.array([R.entropy_of(P[i]) for i in range(n)])
            ok = [bool((np.abs(P[some].sum(axis=1) - 1.0) <= (k + 2) * R.U).all() and (P[~some] == 0).all() and (P[~np.isfinite(d2)] == 0).all()),
                  bool((np.abs(H[conv] - np.log(perp)) <= 2e-5).all()),
                  bool(np.allclose(beta, br, rtol=1e-9) and (np.abs(P - Pr) <= 2 * R.U * Pr + 1e-45).all())]
            bad += not all(ok)
            if verbose:
                print(f"affinities n {n:3d} k {k:2d} perplexity {perp:4.1f} " + "  ".join(f"{n_} {'ok' if v else 'DIFFERS'}" for n_, v in zip(("rows sum to 1", "entropy", "beta and P"), ok)))
        for D in (2, 3):
            c = R.update_case(D=D)
            r = R.update_ref(c)
            n = c["n"]
            rec = call(np.array([2, n, D, len(c["cols"])], np.int32).tobytes() + np.array([c["alpha"], c["momentum"], c["lr"], c["min_gain"]], np.float64).tobytes()
                       + c["indptr"].tobytes() + c["cols"].tobytes() + c["vals"].tobytes() + c["y"].tobytes() + c["u"].tobytes() + c["gain"].tobytes()
                       + c["Zrow"].tobytes() + c["F"].tobytes())
            Z, rest = rec[0], rec[1:]
            grad, kl = rest[:D * n].reshape(D, n), rest[D * n:D * n + n]
            gain, u, y = (rest[D * n + n + s * n * D:D * n + n + (s + 1) * n * D].reshape(n, D) for s in range(3))
            sure = ~r["unsure"]
            ok = [abs(Z - r["Z"]) <= (n + 8) * 2.0 ** -53 * r["Z"], bool((np.abs(grad - r["grad"]) <= r["e_grad"]).all()), bool((np.abs(kl - r["kl_row"]) <= r["e_kl"]).all()),
                  bool((gain[sure] == r["gain"][sure]).all()), bool((np.abs(u - r["u"])[sure] <= r["e_u"][sure]).all() and (np.abs(y - r["y_out"])[sure] <= r["e_y"][sure]).all())]
            bad += not all(ok)
            if verbose:
                print(f"update n {n} D {D} " + "  ".join(f"{n_} {'ok' if v else 'DIFFERS'}" for n_, v in zip(("Z", "gradient", "kl_row", "gains", "u and y"), ok)))
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--cxx", default="g++")
    a = ap.parse_args()
    bad = run(SHAPES[:6] if a.small else SHAPES, AFFINITIES[:2] if a.small else AFFINITIES, a.cxx)
    print("all within bounds" if not bad else f"{bad} case(s) DIFFER")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
