#!/usr/bin/env python3
"""The optimal-transport core on the CPU: compiles the text between the OT-CORE marks of csrc/spv_ot.h -- t of a pair, the online
log-sum-exp update, the merge of two partial states, the order-preserving key -- behind the KNN-CORE text of csrc/spv_knn.h it builds
on (distance chain, unsorted set, sort, merge of lists, chunk plan), as plain C++ with one-line stand-ins for the intrinsics (libm's
correctly rounded fmaf, libm's expf for the device's exp; built with -ffp-contract=off), runs it over a few shapes and compares with
numpy (tests/_ot_reference.py):

  * every pair's t must EQUAL ``t_ref``;
  * L of one scan of the candidates (ot_update per candidate, ot_lse_value) and L through n_split chunks merged in chunk order
    (ot_merge) must lie within the bound of tests/test_gpu_ot.py of the float64 log-sum-exp over the same t;
  * the keys of all candidates with a finite t, sorted as unsigned words, must give numpy's stable sort of (-t, j), and ot_key_t
    must give back t's bits (-0 as +0);
  * the k best of one scan (knn_keep with ot_better, then knn_sort) and of the split-and-merge route must EQUAL ``topk_ref``.
No GPU, nothing loaded into Python.  It checks the arithmetic, the order and the list handling, not the kernels' indexing.

    python tools/ot_host_check.py [--sanitize] [--cxx g++] [--small]

--sanitize builds the program with the address and undefined-behaviour sanitizers (a stand-alone executable with its own main); the
lists are heap blocks of exactly the slots of k entries at stride 3, so a slot written outside one is reported.  --small: the first shapes only."""
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
#include <vector>
#define __host__
#define __device__
#define __forceinline__ inline
static inline float __fsub_rn(float a, float b) { return a - b; }
static inline float __fmaf_rn(float a, float b, float c) { return fmaf(a, b, c); }
static inline float ot_exp(float x) { return expf(x); }
"""
MAIN = """
constexpr int ST = 3;   // list stride: the kernels' lists are strided too
struct List {           // a heap block of exactly knn_slots(k) keys at stride ST: the sanitizer sees any slot beyond it
  knn_key_t* key; int k;
  explicit List(int k_) : key((knn_key_t*)malloc(sizeof(knn_key_t) * ((knn_slots(k_) - 1) * ST + 1))), k(k_) { ot_clear(key, ST, k); knn_pad(key, ST, k); }
  ~List() { free(key); }
  void scan(const float* t, int c0, int c1) {   // what a lane does with its chunk
    KnnTop top;
    ot_top_init(top);
    for (int c = c0; c < c1; ++c)
      if (ot_better(t[c], c, top.worst)) knn_keep(top, key, ST, k, ot_key(t[c], c));
    knn_sort(key, ST, top.fill);
  }
};
static OtLse lse_scan(const float* t, int c0, int c1) {
  OtLse a;
  ot_lse_init(a);
  for (int c = c0; c < c1; ++c) ot_update(a, t[c]);
  return a;
}

int main(int argc, char** argv) {   // argv: input file, output file
  FILE* f = fopen(argv[1], "rb"); FILE* o = fopen(argv[2], "wb");
  if (!f || !o) return 2;
  int h[5]; float s;   // n_q, n_c, D, k, n_split; s
  if (fread(h, 4, 5, f) != 5 || fread(&s, 4, 1, f) != 1) return 3;
  const int n_q = h[0], n_c = h[1], D = h[2], k = h[3], n_split = h[4];
  std::vector<float> Q((size_t)n_q * D), C((size_t)n_c * D + 1), hv(n_c + 1);
  if (fread(Q.data(), 4, Q.size(), f) != Q.size() || fread(C.data(), 4, (size_t)n_c * D, f) != (size_t)n_c * D || fread(hv.data(), 4, n_c, f) != (size_t)n_c) return 3;
  std::vector<float> t(n_c + 1), back(n_c + 1), pt(k); std::vector<int> pj(k); std::vector<knn_key_t> keys(n_c + 1), part_keys(k);
  const int per = knn_chunk(n_c, n_split);
  for (int i = 0; i < n_q; ++i) {
    const float* q = Q.data() + (size_t)i * D;
    for (int c = 0; c < n_c; ++c) {
      t[c] = ot_t(knn_d2(q, C.data() + (size_t)c * D, D), s, hv[c]);
      keys[c] = ot_finite(t[c]) ? ot_key(t[c], c) : OT_EMPTY;
      back[c] = ot_finite(t[c]) ? ot_key_t(keys[c]) : 0.f;
    }
    fwrite(t.data(), 4, n_c, o); fwrite(keys.data(), 8, n_c, o); fwrite(back.data(), 4, n_c, o);
    float L[2];
    L[0] = ot_lse_value(lse_scan(t.data(), 0, n_c));
    OtLse m;
    ot_lse_init(m);
    List one(k), merged(k);
    one.scan(t.data(), 0, n_c);
    for (int c = 0; c < n_split; ++c) {
      const long first = (long)c * per;
      const int c0 = first < n_c ? (int)first : n_c, c1 = first + per < n_c ? (int)(first + per) : n_c;
      ot_merge(m, lse_scan(t.data(), c0, c1));
      List part(k);
      part.scan(t.data(), c0, c1);
      for (int e = 0; e < k; ++e) part_keys[e] = part.key[e * ST];
      knn_merge(merged.key, ST, k, part_keys.data());
    }
    L[1] = ot_lse_value(m);
    fwrite(L, 4, 2, o);
    for (List* l : {&one, &merged}) {
      for (int e = 0; e < k; ++e) {
        const knn_key_t key = l->key[e * ST];
        pj[e] = ot_key_empty(key) ? -1 : knn_key_j(key);
        pt[e] = ot_key_empty(key) ? 0.f : ot_key_t(key);
      }
      fwrite(pj.data(), 4, k, o); fwrite(pt.data(), 4, k, o);
    }
  }
  fclose(o); fclose(f); return 0;
}
"""
# (n_q, n_c, D, k, n_split, data, s): lattice data makes ties plentiful, "edge" puts -inf / nan / +inf among h and huge rows among the candidates
SHAPES = [(5, 40, 3, 4, 3, "lattice", 0.5), (7, 9, 1, 16, 12, "lattice", 1.0), (3, 0, 4, 2, 2, "real", 1.0), (6, 70, 25, 15, 7, "edge", 0.4),
          (9, 300, 35, 64, 5, "real", 0.3), (8, 120, 25, 17, 64, "edge", 2.0), (4, 257, 64, 1, 2, "real", 0.05), (12, 500, 10, 50, 1, "lattice", 3.0)]


def host_source() -> str:
    """the two cores as they stand in the headers, between the stand-ins and a main()"""
    knn = open(os.path.join(ROOT, "spvipes_amd", "csrc", "spv_knn.h")).read()
    ot = open(os.path.join(ROOT, "spvipes_amd", "csrc", "spv_ot.h")).read()
    return (SHIMS + knn[knn.index("// ---- KNN-CORE-BEGIN ----"):knn.index("// ---- KNN-CORE-END ----")]
            + ot[ot.index("// ---- OT-CORE-BEGIN ----"):ot.index("// ---- OT-CORE-END ----")] + MAIN)


def make_case(rng, n_q, n_c, D, kind):
    if kind == "lattice":
        Q, C = (rng.integers(-32, 33, (n, D)).astype(np.float32) / 4 for n in (n_q, n_c))
        h = rng.integers(-8, 9, n_c).astype(np.float32) / 2   # t exact, ties across different costs too; zeros of both signs below
        h[h == 0] = np.where(rng.random(int((h == 0).sum())) < 0.5, np.float32(-0.0), np.float32(0.0))
    else:
        Q, C = (rng.standard_normal((n, D)).astype(np.float32) for n in (n_q, n_c))
        h = rng.standard_normal(n_c).astype(np.float32)
    if kind == "edge" and n_c >= 12:
        C[1, 0], C[3, :], C[5, 2], C[6, :] = np.inf, np.nan, -np.inf, 3e19   # (3e19)^2 * D overflows float32: t = -inf
        C[7] = Q[0]                                                          # cost +0
        h[8], h[9], h[10], h[11] = -np.inf, np.nan, np.inf, -0.0
    return Q, C, h


def lse_bound(L_ref, n_chain, n_split, n_c):
    """the bound of tests/test_gpu_ot.py (derived there)"""
    return (3 * n_chain + 4 * n_split + 5 * np.log(n_c + 1.0) + 16) * 2.0 ** -24 + 2.0 ** -23 * np.maximum(np.abs(L_ref), 1.0)


def run(shapes, sanitize=False, cxx="g++", verbose=True) -> int:
    from tests._ot_reference import lse_ref, t_ref, topk_ref
    bad = 0
    rng = np.random.default_rng(11)
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "ot_host.cpp"), os.path.join(d, "ot_host")
        open(src, "w").write(host_source())
        subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", *(["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []),
                        "-o", exe, src], check=True)
        for n_q, n_c, D, k, n_split, kind, s in shapes:
            Q, C, h = make_case(rng, n_q, n_c, D, kind)
            fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
            with open(fin, "wb") as f:
                f.write(np.array([n_q, n_c, D, k, n_split], np.int32).tobytes() + np.float32(s).tobytes() + Q.tobytes() + C.tobytes() + h.tobytes())
            subprocess.run([exe, fin, fout], check=True)
            rec = np.fromfile(fout, np.uint32).reshape(n_q, 4 * n_c + 2 + 4 * k)
            t = rec[:, :n_c].view(np.float32)
            keys = np.ascontiguousarray(rec[:, n_c:3 * n_c]).view(np.uint64)
            back = rec[:, 3 * n_c:4 * n_c].view(np.float32)
            L = rec[:, 4 * n_c:4 * n_c + 2].view(np.float32).astype(np.float64)
            o = 4 * n_c + 2
            lists = [(rec[:, o + 2 * k * m:o + 2 * k * m + k].view(np.int32), rec[:, o + 2 * k * m + k:o + 2 * k * (m + 1)].view(np.float32)) for m in (0, 1)]
            want_t = t_ref(Q, C, h, s)
            want_L = lse_ref(want_t)
            want_idx, want_tv = topk_ref(want_t, k)
            ok = [np.array_equal(t.view(np.uint32), want_t.view(np.uint32))]
            per = -(-n_c // n_split) if n_c else 0
            with np.errstate(invalid="ignore"):
                fin_L = np.isfinite(want_L)
                ok.append(all((np.isneginf(L[~fin_L, m]).all() and (np.abs(L[fin_L, m] - want_L[fin_L]) <= lse_bound(want_L[fin_L], nc, ns, n_c)).all())
                              for m, nc, ns in ((0, n_c, 1), (1, per, n_split))))
            order_ok = True
            for i in range(n_q):
                cand = np.flatnonzero(np.isfinite(want_t[i]))
                by_key = cand[np.argsort(keys[i][cand], kind="stable")]
                order_ok &= np.array_equal(by_key, cand[np.lexsort((cand, -want_t[i][cand].astype(np.float64)))])
                order_ok &= len(np.unique(keys[i][cand])) == len(cand)
                order_ok &= np.array_equal(back[i][cand].view(np.uint32), (want_t[i][cand] + np.float32(0)).view(np.uint32))
            ok.append(bool(order_ok))
            for idx, tv in lists:
                filled = want_idx >= 0
                ok.append(np.array_equal(idx, want_idx) and np.array_equal(tv[filled].view(np.uint32), (want_tv[filled] + np.float32(0)).view(np.uint32)))
            bad += not all(ok)
            if verbose:
                names = ("t", "log-sum-exp", "key order", "one scan", "split and merge")
                print(f"n_q {n_q:3d} n_c {n_c:3d} D {D:2d} k {k:2d} n_split {n_split:2d} {kind:8s} " + "  ".join(f"{n} {'ok' if v else 'DIFFERS'}" for n, v in zip(names, ok)))
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sanitize", action="store_true")
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--cxx", default="g++")
    a = ap.parse_args()
    bad = run(SHAPES[:4] if a.small else SHAPES, a.sanitize, a.cxx)
    print("all within bounds" if not bad else f"{bad} shape(s) DIFFER")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
