#!/usr/bin/env python3
"""The paged nearest-neighbour search and the LISI core on the CPU: compiles the text between the KNN-CORE marks of csrc/spv_knn.h (the
paging predicate knn_after with the list handling it sits in) and between the LISI-CORE marks of csrc/spv_lisi.h (the lane sums, the
entropy, the search's update, the affinities and the Simpson step), exactly as the kernels use them, as plain C++ with one-line stand-ins
for the rounding intrinsics (-ffp-contract=off; libm's fmaf and sqrtf are correctly rounded), and holds them to the float64 numpy
reference (tests/_lisi_reference.py):

  * paging: per query, page after page -- a scan of every chunk that offers only the candidates AFTER the previous page's last key, the
    sort, the merge in chunk order -- must EQUAL ``paged_ref`` (np.lexsort on (d, j)), indices and distance bits, ties that straddle
    the page boundaries, the fill and the exclusion included;
  * LISI: the 64 lanes of a row and the butterfly are played in the kernel's order; beta must match the reference's to rtol 1e-6 and the
    entropy at it the target within 2e-5 on the rows the reference converges on, ``converged`` and ``n_valid`` must equal it, and lisi must
    match the reference evaluated at the program's OWN beta within (8 k + 8) 2^-53 relative (``lisi_bound`` derives it).
No GPU, nothing loaded into Python.  It checks the arithmetic, the order and the list handling, not the kernels' indexing.

    python tools/lisi_host_check.py [--sanitize] [--cxx g++] [--small]

--sanitize builds the program with the address and undefined-behaviour sanitizers (a stand-alone executable with its own main); the lists
are heap blocks of exactly the slots of a page at stride 3, and the rows' p / code arrays are heap blocks of exactly k entries."""
import argparse
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np

from tools.knn_host_check import SHIMS, make_case

MAIN = """
constexpr int ST = 3;
struct List {
  knn_key_t* key; int k;
  explicit List(int k_) : key((knn_key_t*)malloc(sizeof(knn_key_t) * ((knn_slots(k_) - 1) * ST + 1))), k(k_) { knn_clear(key, ST, k); knn_pad(key, ST, k); }
  ~List() { free(key); }
  void scan(const float* q, const float* C, int D, int c0, int c1, int ex, bool paged, knn_key_t after) {   // what a lane does with its chunk
    KnnTop top;
    knn_top_init(top);
    for (int c = c0; c < c1; ++c) {
      const float v = knn_d2(q, C + (size_t)c * D, D);
      if (c != ex && knn_better(v, c, top.worst) && (!paged || knn_after(v, c, after))) knn_keep(top, key, ST, k, knn_key(v, c));
    }
    knn_sort(key, ST, top.fill);
  }
};

static double fold(double* x) {   // the butterfly: x[l] += x[l ^ m] for m = 32 .. 1; every lane ends with the same bits
  for (int m = LISI_LANES / 2; m >= 1; m /= 2) {
    double y[LISI_LANES];
    for (int l = 0; l < LISI_LANES; ++l) y[l] = x[l] + x[l ^ m];
    for (int l = 0; l < LISI_LANES; ++l) x[l] = y[l];
  }
  for (int l = 1; l < LISI_LANES; ++l) if (memcmp(&x[l], &x[0], 8)) abort();
  return x[0];
}

static int paging(FILE* f, FILE* o) {
  int h[6];   // n_q, n_c, D, k, n_split, has_exclude
  if (fread(h, 4, 6, f) != 6) return 3;
  const int n_q = h[0], n_c = h[1], D = h[2], k = h[3], n_split = h[4];
  std::vector<float> Q((size_t)n_q * D), C((size_t)n_c * D + 1);
  std::vector<int> ex(n_q, -1);
  if (fread(Q.data(), 4, Q.size(), f) != Q.size() || fread(C.data(), 4, (size_t)n_c * D, f) != (size_t)n_c * D) return 3;
  if (h[5] && fread(ex.data(), 4, n_q, f) != (size_t)n_q) return 3;
  const int per = knn_chunk(n_c, n_split);
  for (int i = 0; i < n_q; ++i) {
    const float* q = Q.data() + (size_t)i * D;
    float* dist = (float*)malloc(4 * k); int* idx = (int*)malloc(4 * k);   // the row as the entry point writes it: exactly k columns
    for (int page = 0; page * KNN_KMAX < k; ++page) {
      const int c0 = page * KNN_KMAX, kp = knn_page_cols(k, page);
      const knn_key_t after = page ? knn_after_key(dist[c0 - 1], idx[c0 - 1]) : KNN_EMPTY;
      List merged(kp);
      std::vector<knn_key_t> part_keys(kp);
      for (int s = 0; s < n_split; ++s) {
        const long first = (long)s * per;
        List part(kp);
        part.scan(q, C.data(), D, first < n_c ? (int)first : n_c, first + per < n_c ? (int)(first + per) : n_c, ex[i], page > 0, after);
        for (int e = 0; e < kp; ++e) part_keys[e] = part.key[e * ST];
        knn_merge(merged.key, ST, kp, part_keys.data());
      }
      for (int e = 0; e < kp; ++e) { dist[c0 + e] = knn_key_d(merged.key[e * ST]); idx[c0 + e] = knn_key_j(merged.key[e * ST]); }
    }
    fwrite(idx, 4, k, o); fwrite(dist, 4, k, o);
    free(dist); free(idx);
  }
  return 0;
}

static int lisi(FILE* f, FILE* o) {
  int h[4];   // n, k, n_c, n_sets
  double perplexity;
  if (fread(h, 4, 4, f) != 4 || fread(&perplexity, 8, 1, f) != 1) return 3;
  const int n = h[0], k = h[1], n_c = h[2], n_sets = h[3];
  std::vector<int> idx((size_t)n * k), codes((size_t)n_sets * n_c + 1);
  std::vector<float> dist((size_t)n * k);
  if (fread(idx.data(), 4, idx.size(), f) != idx.size() || fread(dist.data(), 4, dist.size(), f) != dist.size()
      || fread(codes.data(), 4, (size_t)n_sets * n_c, f) != (size_t)n_sets * n_c) return 3;
  const double log_perp = log(perplexity);
  for (int i = 0; i < n; ++i) {
    const float* d2 = dist.data() + (size_t)i * k;
    const bool any = d2[0] < INFINITY;
    const double r0 = lisi_root(d2[0]);
    double d[LISI_LANES][LISI_SLOTS];
    int cnt = 0;
    for (int l = 0; l < LISI_LANES; ++l)
      for (int m = 0; m < LISI_SLOTS; ++m) {
        const int j = l + m * LISI_LANES;
        const bool ok = any && j < k && d2[j] < INFINITY;
        d[l][m] = ok ? lisi_root(d2[j]) - r0 : -1.0;
        if (ok && !(d[l][m] >= 0.0)) d[l][m] = 0.0;
        cnt += ok;
      }
    double beta = 1.0, S = 1.0, out_beta;
    int conv = 0;
    if (any) {
      double lo = -INFINITY, hi = INFINITY, T, diff, Sl[LISI_LANES], Tl[LISI_LANES];
      for (int tries = 0;; ++tries) {
        for (int l = 0; l < LISI_LANES; ++l) lisi_lane_sums(d[l], beta, Sl[l], Tl[l]);
        S = fold(Sl);
        T = fold(Tl);
        diff = lisi_entropy(S, T, beta) - log_perp;
        if (fabs(diff) < LISI_TOL || tries == LISI_STEPS) break;
        lisi_update(diff, beta, lo, hi);
      }
      conv = fabs(diff) < LISI_TOL;
    }
    out_beta = beta;
    fwrite(&out_beta, 8, 1, o); fwrite(&cnt, 4, 1, o); fwrite(&conv, 4, 1, o);
    double* p = (double*)malloc(8 * k); int* code = (int*)malloc(4 * k);   // exactly k entries: the sanitizer sees a slot beyond them
    for (int j = 0; j < k; ++j) p[j] = any ? lisi_p(d[j % LISI_LANES][j / LISI_LANES], beta, S) : 0.0;
    for (int t = 0; t < n_sets; ++t) {
      for (int j = 0; j < k; ++j) {
        const int nb = (any && d2[j] < INFINITY) ? idx[(size_t)i * k + j] : -1;
        code[j] = (nb >= 0 && nb < n_c) ? codes[(size_t)t * n_c + nb] : -1;
      }
      double v[LISI_LANES];
      for (int l = 0; l < LISI_LANES; ++l) v[l] = lisi_lane_simpson(p, code, k, l);
      const double simpson = fold(v), res = any ? 1.0 / simpson : NAN;
      fwrite(&res, 8, 1, o);
    }
    free(p); free(code);
  }
  return 0;
}

int main(int argc, char** argv) {   // argv: "paging" | "lisi", input file, output file
  if (argc != 4) return 2;
  FILE* f = fopen(argv[2], "rb"); FILE* o = fopen(argv[3], "wb");
  if (!f || !o) return 2;
  const int rc = argv[1][0] == 'p' ? paging(f, o) : lisi(f, o);
  fclose(o); fclose(f);
  return rc;
}
"""
# (n_q, n_c, D, k, n_split, data, exclude): D = 1 / 2 lattices put hundreds of ties across the places 64 / 65 and 128 / 129
PAGING = [(5, 300, 1, 130, 3, "lattice", False), (4, 200, 2, 65, 1, "lattice", True), (3, 70, 3, 256, 2, "real", False), (6, 300, 25, 89, 7, "real", True),
          (2, 0, 4, 70, 2, "real", False), (4, 130, 25, 129, 64, "edge", True), (3, 700, 2, 256, 5, "lattice", True), (5, 64, 10, 64, 2, "real", False)]
# (n, k, n_c, n_sets, perplexity)
LISI = [(6, 89, 200, 2, 30.0), (5, 1, 10, 1, 1.0), (7, 64, 90, 8, 20.0), (4, 256, 300, 3, 85.0), (5, 65, 70, 2, 5.0), (6, 2, 9, 1, 30.0)]


def host_source() -> str:
    """the two cores as they stand in the headers, between the stand-ins and a main()"""
    knn = open(os.path.join(ROOT, "spvipes_amd", "csrc", "spv_knn.h")).read()
    lisi = open(os.path.join(ROOT, "spvipes_amd", "csrc", "spv_lisi.h")).read()
    return (SHIMS + "#include <cstring>\n" + knn[knn.index("// ---- KNN-CORE-BEGIN ----"):knn.index("// ---- KNN-CORE-END ----")]
            + lisi[lisi.index("// ---- LISI-CORE-BEGIN ----"):lisi.index("// ---- LISI-CORE-END ----")] + MAIN)


def run(small=False, sanitize=False, cxx="g++", verbose=True) -> int:
    from tests._lisi_reference import lisi_bound, lisi_ref, make_lists, paged_ref
    bad = 0
    rng = np.random.default_rng(11)
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "lisi_host.cpp"), os.path.join(d, "lisi_host")
        open(src, "w").write(host_source())
        subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", *(["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []),
                        "-o", exe, src], check=True)
        fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        for n_q, n_c, D, k, n_split, kind, with_ex in (PAGING[:3] if small else PAGING):
            Q, C, ex = make_case(rng, n_q, n_c, D, kind, with_ex)
            with open(fin, "wb") as f:
                f.write(np.array([n_q, n_c, D, k, n_split, int(ex is not None)], np.int32).tobytes() + Q.tobytes() + C.tobytes() + (ex.tobytes() if ex is not None else b""))
            subprocess.run([exe, "paging", fin, fout], check=True)
            rec = np.fromfile(fout, np.uint32).reshape(n_q, 2 * k)
            want = paged_ref(Q, C, k, ex)
            ok = np.array_equal(rec[:, :k].view(np.int32), want[0]) and np.array_equal(rec[:, k:], want[1].view(np.uint32))
            ties = [int((want[1][:, c - 1] == want[1][:, c]).sum()) for c in (64, 128) if c < k]
            bad += not ok
            if verbose:
                print(f"paging n_q {n_q:2d} n_c {n_c:3d} D {D:2d} k {k:3d} n_split {n_split:2d} {kind:8s} ties across the page boundaries {ties}  {'ok' if ok else 'DIFFERS'}")
        for n, k, n_c, n_sets, perp in (LISI[:3] if small else LISI):
            idx, dist, codes = make_lists(rng, n, k, n_c, n_sets)
            with open(fin, "wb") as f:
                f.write(np.array([n, k, n_c, n_sets], np.int32).tobytes() + np.float64(perp).tobytes() + idx.tobytes() + dist.tobytes() + codes.tobytes())
            subprocess.run([exe, "lisi", fin, fout], check=True)
            rec = np.frombuffer(open(fout, "rb").read(), dtype=np.dtype([("beta", "<f8"), ("n_valid", "<i4"), ("conv", "<i4"), ("lisi", "<f8", (n_sets,))]))
            ref = lisi_ref(idx, dist, codes, perp)
            at = lisi_ref(idx, dist, codes, perp, beta=rec["beta"])
            on = ref[3]
            ok = [np.array_equal(rec["n_valid"], ref[2]), np.array_equal(rec["conv"].astype(bool), ref[3]),
                  np.allclose(rec["beta"][on], ref[1][on], rtol=1e-6, atol=0), bool((np.abs(at[4][on] - np.log(perp)) <= 2e-5).all()),
                  np.array_equal(np.isnan(rec["lisi"].T), np.isnan(at[0]))]
            fin_ = np.isfinite(at[0])
            err = float(np.max(np.abs(rec["lisi"].T[fin_] / at[0][fin_] - 1), initial=0.0))
            ok.append(err <= lisi_bound(k) and np.array_equal(rec["lisi"].T[~fin_ & ~np.isnan(at[0])], at[0][~fin_ & ~np.isnan(at[0])]))
            bad += not all(ok)
            if verbose:
                print(f"lisi n {n:2d} k {k:3d} n_c {n_c:3d} sets {n_sets} perplexity {perp:5.1f} converged {int(on.sum())}/{n}  largest relative deviation {err:.2e} "
                      f"(bound {lisi_bound(k):.2e})  {'ok' if all(ok) else 'DIFFERS ' + str(ok)}")
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sanitize", action="store_true")
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--cxx", default="g++")
    a = ap.parse_args()
    bad = run(a.small, a.sanitize, a.cxx)
    print("all hold" if not bad else f"{bad} case(s) DIFFER")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
