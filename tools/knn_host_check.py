#!/usr/bin/env python3
"""The nearest-neighbour core on the CPU: compiles the text between the KNN-CORE marks of csrc/spv_knn.h -- the per-pair distance chain,
the (d, j) keys, the scan's unsorted set, the final sort, the merge of chunk lists and the chunk plan, exactly as the kernels use them -- as plain
C++ with two one-line stand-ins for the rounding intrinsics (a subtraction and libm's correctly rounded fmaf, built with
-ffp-contract=off), runs it over a few shapes and compares with numpy (tests/_knn_reference.py):

  * every pair's distance must EQUAL ``exact_d2``;
  * the k best of one scan of the candidates (knn_keep, then knn_sort) must EQUAL ``knn_ref`` (indices and distances, ties and fill included);
  * the same through n_split chunks (chunks without a candidate included), each scanned into a list of its own, then merged in
    chunk order, must equal it too.
No GPU, nothing loaded into Python.  It checks the arithmetic, the order and the list handling, not the kernels' indexing.

    python tools/knn_host_check.py [--sanitize] [--cxx g++] [--small]

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
"""
MAIN = """
constexpr int ST = 3;   // list stride: the kernels' lists are strided too
struct List {           // a heap block of exactly knn_slots(k) keys at stride ST: the sanitizer sees any slot beyond it
  knn_key_t* key; int k;
  explicit List(int k_) : key((knn_key_t*)malloc(sizeof(knn_key_t) * ((knn_slots(k_) - 1) * ST + 1))), k(k_) { knn_clear(key, ST, k); knn_pad(key, ST, k); }
  ~List() { free(key); }
  void scan(const float* q, const float* C, int D, int c0, int c1, int ex) {   // what a lane does with its chunk
    KnnTop top;
    knn_top_init(top);
    for (int c = c0; c < c1; ++c) {
      const float v = knn_d2(q, C + (size_t)c * D, D);
      if (c != ex && knn_better(v, c, top.worst)) knn_keep(top, key, ST, k, knn_key(v, c));
    }
    knn_sort(key, ST, top.fill);
  }
};

int main(int argc, char** argv) {   // argv: input file, output file
  FILE* f = fopen(argv[1], "rb"); FILE* o = fopen(argv[2], "wb");
  if (!f || !o) return 2;
  int h[6];   // n_q, n_c, D, k, n_split, has_exclude
  if (fread(h, 4, 6, f) != 6) return 3;
  const int n_q = h[0], n_c = h[1], D = h[2], k = h[3], n_split = h[4];
  std::vector<float> Q((size_t)n_q * D), C((size_t)n_c * D + 1);
  std::vector<int> ex(n_q, -1);
  if (fread(Q.data(), 4, Q.size(), f) != Q.size() || fread(C.data(), 4, (size_t)n_c * D, f) != (size_t)n_c * D) return 3;
  if (h[5] && fread(ex.data(), 4, n_q, f) != (size_t)n_q) return 3;
  std::vector<float> row(n_c + 1), pd(k); std::vector<int> pj(k); std::vector<knn_key_t> part_keys(k);
  const int per = knn_chunk(n_c, n_split);
  for (int i = 0; i < n_q; ++i) {
    const float* q = Q.data() + (size_t)i * D;
    for (int c = 0; c < n_c; ++c) row[c] = knn_d2(q, C.data() + (size_t)c * D, D);
    fwrite(row.data(), 4, n_c, o);
    List one(k), merged(k);
    one.scan(q, C.data(), D, 0, n_c, ex[i]);
    for (int s = 0; s < n_split; ++s) {
      const long first = (long)s * per;
      List part(k);
      part.scan(q, C.data(), D, first < n_c ? (int)first : n_c, first + per < n_c ? (int)(first + per) : n_c, ex[i]);
      for (int e = 0; e < k; ++e) part_keys[e] = part.key[e * ST];
      knn_merge(merged.key, ST, k, part_keys.data());
    }
    for (List* l : {&one, &merged}) {
      for (int e = 0; e < k; ++e) { pd[e] = knn_key_d(l->key[e * ST]); pj[e] = knn_key_j(l->key[e * ST]); }
      fwrite(pj.data(), 4, k, o); fwrite(pd.data(), 4, k, o);
    }
  }
  const int shapes[][2] = {{50000, 50000}, {100000, 100000}, {1, 1000000}, {300, 260}, {65536, 10}, {1, 0}};
  for (auto& s : shapes) printf("knn_splits(%d, %d) = %d\\n", s[0], s[1], knn_splits(s[0], s[1]));
  fclose(o); fclose(f); return 0;
}
"""
# (n_q, n_c, D, k, n_split, data, exclude): lattice data makes ties plentiful, "edge" puts inf / nan / huge rows among the candidates
SHAPES = [(5, 40, 3, 4, 3, "lattice", True), (7, 9, 1, 16, 12, "lattice", False), (3, 0, 4, 2, 2, "real", False), (6, 70, 25, 15, 7, "real", True),
          (9, 300, 35, 64, 5, "real", False), (8, 120, 25, 17, 64, "edge", True), (4, 257, 64, 1, 2, "real", False), (12, 500, 10, 50, 1, "lattice", True)]


def host_source() -> str:
    """the core as it stands in the header, between the stand-ins and a main()"""
    text = open(os.path.join(ROOT, "spvipes_amd", "csrc", "spv_knn.h")).read()
    return SHIMS + text[text.index("// ---- KNN-CORE-BEGIN ----"):text.index("// ---- KNN-CORE-END ----")] + MAIN


def make_case(rng, n_q, n_c, D, kind, with_exclude):
    if kind == "lattice":
        Q, C = (rng.integers(-32, 33, (n, D)).astype(np.float32) / 4 for n in (n_q, n_c))
    else:
        Q, C = (rng.standard_normal((n, D)).astype(np.float32) for n in (n_q, n_c))
    if kind == "edge" and n_c >= 8:
        C[1, 0], C[3, :], C[5, 2], C[6, :] = np.inf, np.nan, -np.inf, 3e19   # (3e19)^2 * D overflows float32
        C[7] = Q[0]                                                          # distance +0
    ex = rng.integers(-2, n_c + 2, n_q).astype(np.int32) if with_exclude else None
    return Q, C, ex


def run(shapes, sanitize=False, cxx="g++", verbose=True) -> int:
    from tests._knn_reference import exact_d2, knn_ref
    bad = 0
    rng = np.random.default_rng(7)
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "knn_host.cpp"), os.path.join(d, "knn_host")
        open(src, "w").write(host_source())
        subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", *(["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []),
                        "-o", exe, src], check=True)
        for n_q, n_c, D, k, n_split, kind, with_ex in shapes:
            Q, C, ex = make_case(rng, n_q, n_c, D, kind, with_ex)
            fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
            with open(fin, "wb") as f:
                f.write(np.array([n_q, n_c, D, k, n_split, int(ex is not None)], np.int32).tobytes() + Q.tobytes() + C.tobytes() + (ex.tobytes() if ex is not None else b""))
            res = subprocess.run([exe, fin, fout], check=True, capture_output=True, text=True)
            rec = np.fromfile(fout, np.uint32).reshape(n_q, n_c + 4 * k)
            d2 = rec[:, :n_c].view(np.float32)
            lists = [(rec[:, n_c + 2 * k * m:n_c + 2 * k * m + k].view(np.int32), rec[:, n_c + 2 * k * m + k:n_c + 2 * k * (m + 1)].view(np.float32)) for m in (0, 1)]
            want_d2 = exact_d2(Q, C)
            want = knn_ref(Q, C, k, ex, d2=want_d2)
            ok = [np.array_equal(d2.view(np.uint32), want_d2.view(np.uint32))]
            ok += [np.array_equal(i, want[0]) and np.array_equal(v.view(np.uint32), want[1].view(np.uint32)) for i, v in lists]
            bad += not all(ok)
            if verbose:
                print(f"n_q {n_q:3d} n_c {n_c:3d} D {D:2d} k {k:2d} n_split {n_split:2d} {kind:8s} distances {'ok' if ok[0] else 'DIFFER'}  one scan {'ok' if ok[1] else 'DIFFERS'}"
                      f"  split and merge {'ok' if ok[2] else 'DIFFERS'}")
        if verbose:
            print(res.stdout, end="")
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sanitize", action="store_true")
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--cxx", default="g++")
    a = ap.parse_args()
    bad = run(SHAPES[:4] if a.small else SHAPES, a.sanitize, a.cxx)
    print("all equal" if not bad else f"{bad} shape(s) DIFFER")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
