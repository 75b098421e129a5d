#!/usr/bin/env python3
"""The silhouette core on the CPU: compiles the text between the SIL-CORE marks of csrc/spv_silhouette.h -- the per-candidate step, the
walk over the segment boundaries, the merge of the chunks' partial sums, the chunk plan and the workspace size, exactly as the kernels use
them -- after the KNN-CORE text of csrc/spv_knn.h it builds on, as plain C++ with two one-line stand-ins for the rounding intrinsics (built
with -ffp-contract=off; libm's sqrtf is the correctly rounded root), runs it over a few shapes and compares with numpy:

  * every pair's distance must EQUAL the float32 root of ``exact_d2`` (tests/_silhouette_reference.distances_ref);
  * one walk over all candidates (sil_advance / sil_add / sil_finish) must EQUAL the float64 sums added in ascending candidate order;
  * the same through n_split chunks (chunks without a candidate included), each walked into a slab of its own, then sil_merge in chunk
    order, must equal the sums added in that grouping.
Both comparisons are bit for bit (``segment_sums_ref(..., n_split=)``: numpy's cumulative sum adds in sequence, like the walk).  No GPU, nothing loaded into Python.  It
checks the arithmetic, the order and the boundary handling, not the kernels' indexing.

    python tools/silhouette_host_check.py [--sanitize] [--cxx g++] [--small]

--sanitize builds the program with the address and undefined-behaviour sanitizers (a stand-alone executable with its own main); a lane's
column is a heap block of exactly n_seg doubles at stride 3, so a sum written outside it is reported.  --small: the first shapes only."""
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
constexpr long ST = 3;   // column stride: the kernels' columns are strided too
struct Column {          // a heap block of exactly n_seg doubles at stride ST: the sanitizer sees any sum beyond it
  double* v; int n_seg;
  explicit Column(int n) : v((double*)malloc(sizeof(double) * ((n - 1) * ST + 1))), n_seg(n) {}
  ~Column() { free(v); }
  void walk(const float* q, const float* C, int D, int c0, int c1, const int* seg_ptr) {   // what a lane does with its chunk
    SilWalk w;
    sil_walk_init(w, seg_ptr);
    for (int j = c0; j < c1; ++j) {
      sil_advance(w, j, seg_ptr, n_seg, v, ST, true);
      sil_add(w, knn_d2(q, C + (size_t)j * D, D));
    }
    sil_finish(w, n_seg, v, ST, true);
  }
};

int main(int argc, char** argv) {   // argv: input file, output file
  FILE* f = fopen(argv[1], "rb"); FILE* o = fopen(argv[2], "wb");
  if (!f || !o) return 2;
  int h[5];   // n_q, n_c, D, n_seg, n_split
  if (fread(h, 4, 5, f) != 5) return 3;
  const int n_q = h[0], n_c = h[1], D = h[2], n_seg = h[3], n_split = h[4];
  std::vector<float> Q((size_t)n_q * D), C((size_t)n_c * D + 1);
  std::vector<int> seg_ptr(n_seg + 1);
  if (fread(Q.data(), 4, Q.size(), f) != Q.size() || fread(C.data(), 4, (size_t)n_c * D, f) != (size_t)n_c * D) return 3;
  if (fread(seg_ptr.data(), 4, n_seg + 1, f) != (size_t)n_seg + 1) return 3;
  std::vector<float> row(n_c + 1);
  std::vector<double> one_out(n_seg), merged_out(n_seg), ws((size_t)n_split * n_seg);
  const int per = knn_chunk(n_c, n_split);
  for (int i = 0; i < n_q; ++i) {
    const float* q = Q.data() + (size_t)i * D;
    for (int c = 0; c < n_c; ++c) row[c] = sil_root(knn_d2(q, C.data() + (size_t)c * D, D));
    fwrite(row.data(), 4, n_c, o);
    Column one(n_seg);
    one.walk(q, C.data(), D, 0, n_c, seg_ptr.data());
    for (int s = 0; s < n_seg; ++s) one_out[s] = one.v[s * ST];
    for (int c = 0; c < n_split; ++c) {
      const long first = (long)c * per;
      Column part(n_seg);
      part.walk(q, C.data(), D, first < n_c ? (int)first : n_c, first + per < n_c ? (int)(first + per) : n_c, seg_ptr.data());
      for (int s = 0; s < n_seg; ++s) ws[(size_t)c * n_seg + s] = part.v[s * ST];   // [chunk][segment], one query
    }
    for (int s = 0; s < n_seg; ++s) merged_out[s] = sil_merge(ws.data() + s, n_seg, n_split);
    fwrite(one_out.data(), 8, n_seg, o); fwrite(merged_out.data(), 8, n_seg, o);
  }
  const int shapes[][2] = {{50000, 50000}, {100000, 100000}, {1, 1000000}, {560, 560}, {65536, 10}, {1, 0}};
  for (auto& s : shapes) printf("sil_splits(%d, %d) = %d\\n", s[0], s[1], sil_splits(s[0], s[1]));
  printf("sil_ws_bytes(2000000, 256, 64) = %lld\\n", sil_ws_bytes(2000000, 256, 64));
  fclose(o); fclose(f); return 0;
}
"""
# (n_q, n_c, D, segment sizes, n_split, data): "edge" puts inf / nan / huge rows among the candidates and a copy of a query
SHAPES = [(5, 40, 3, [0, 7, 1, 0, 0, 20, 12, 0], 3, "lattice"), (7, 9, 1, [9], 12, "real"), (3, 0, 4, [0, 0], 2, "real"),
          (6, 70, 25, [1] * 10 + [60], 7, "real"), (9, 300, 35, [64, 64, 22, 150], 5, "real"), (8, 120, 25, [2, 2, 50, 66], 64, "edge"),
          (4, 257, 64, [1] + [0] * 254 + [256], 2, "real"), (12, 500, 10, [125] * 4, 1, "scales")]


def host_source() -> str:
    """the two cores as they stand in the headers, between the stand-ins and a main()"""
    knn = open(os.path.join(ROOT, "spvipes_amd", "csrc", "spv_knn.h")).read()
    sil = open(os.path.join(ROOT, "spvipes_amd", "csrc", "spv_silhouette.h")).read()
    return (SHIMS + knn[knn.index("// ---- KNN-CORE-BEGIN ----"):knn.index("// ---- KNN-CORE-END ----")]
            + sil[sil.index("// ---- SIL-CORE-BEGIN ----"):sil.index("// ---- SIL-CORE-END ----")] + MAIN)


def make_case(rng, n_q, n_c, D, kind):
    if kind == "lattice":
        Q, C = (rng.integers(-32, 33, (n, D)).astype(np.float32) / 4 for n in (n_q, n_c))
    else:
        Q, C = (rng.standard_normal((n, D)).astype(np.float32) for n in (n_q, n_c))
    if kind == "scales":
        C *= (10.0 ** rng.uniform(-12, 6, (n_c, 1))).astype(np.float32)   # additions that round: the order is what is checked
    if kind == "edge" and n_c >= 8:
        C[1, 0], C[3, :], C[5, 2], C[6, :] = np.inf, np.nan, -np.inf, 3e19   # (3e19)^2 * D overflows float32
        C[7] = Q[0]                                                          # distance +0
    return Q, C


def same_bits(a, b) -> bool:
    """equal bit for bit, a NaN matching any NaN (its sign and payload are not part of the contract)"""
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    return a.shape == b.shape and a.dtype == b.dtype and bool(((np.ascontiguousarray(a).view(u) == np.ascontiguousarray(b).view(u)) | (np.isnan(a) & np.isnan(b))).all())


def run(shapes, sanitize=False, cxx="g++", verbose=True) -> int:
    from tests._silhouette_reference import distances_ref, segment_sums_ref
    bad = 0
    rng = np.random.default_rng(11)
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "sil_host.cpp"), os.path.join(d, "sil_host")
        open(src, "w").write(host_source())
        subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", *(["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []),
                        "-o", exe, src], check=True)
        for n_q, n_c, D, seg_sizes, n_split, kind in shapes:
            Q, C = make_case(rng, n_q, n_c, D, kind)
            seg_ptr = np.concatenate([[0], np.cumsum(seg_sizes)]).astype(np.int32)
            assert seg_ptr[-1] == n_c
            n_seg = len(seg_sizes)
            fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
            with open(fin, "wb") as f:
                f.write(np.array([n_q, n_c, D, n_seg, n_split], np.int32).tobytes() + Q.tobytes() + C.tobytes() + seg_ptr.tobytes())
            res = subprocess.run([exe, fin, fout], check=True, capture_output=True, text=True)
            rec = np.fromfile(fout, np.uint8).reshape(n_q, 4 * n_c + 16 * n_seg)
            dist = np.ascontiguousarray(rec[:, :4 * n_c]).view(np.float32).reshape(n_q, n_c)
            sums = np.ascontiguousarray(rec[:, 4 * n_c:]).view(np.float64).reshape(n_q, 2, n_seg)
            want_d = distances_ref(Q, C)
            ok = [same_bits(dist, want_d), same_bits(sums[:, 0], segment_sums_ref(Q, C, seg_ptr, d=want_d, n_split=1)),
                  same_bits(sums[:, 1], segment_sums_ref(Q, C, seg_ptr, d=want_d, n_split=n_split))]
            bad += not all(ok)
            if verbose:
                print(f"n_q {n_q:3d} n_c {n_c:3d} D {D:2d} n_seg {n_seg:3d} n_split {n_split:2d} {kind:8s} distances {'ok' if ok[0] else 'DIFFER'}  one walk {'ok' if ok[1] else 'DIFFERS'}"
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
