#!/usr/bin/env python3
"""The segmented log-sum-exp core on the CPU: compiles the text between the OTSEG-CORE marks of csrc/spv_ot_segments.h -- the walk over
the segments, the write-out of a state or a value, the finish and the merge of the chunks' states -- behind the KNN-CORE text of
csrc/spv_knn.h and the OT-CORE text of csrc/spv_ot.h it builds on, as plain C++ with ot_host_check.py's one-line stand-ins for the
intrinsics (built with -ffp-contract=off), runs it over a few shapes the way the kernels do (one walk per (query, chunk) in ascending
candidate order, the chunk plan of knn_chunk, the workspace [chunk][segment][query]) and compares with numpy
(tests/_ot_segment_reference.py):

  * L of one chunk (the walk writes ot_lse_value itself) and L through n_split chunks and otseg_merge must lie within the bound of
    tests/test_gpu_ot.py of the float64 log-sum-exp per segment, -inf exactly where the reference is -inf (empty segments, segments
    whose every t is not finite);
  * every slot of L and of the workspace must have been written, none outside them (heap blocks of exactly their sizes);
  * with ONE segment both routes must EQUAL, bit for bit, the plain ot_update / ot_merge / ot_lse_value route of ot_softmin_kernel at
    the same chunk plan;
  * a seg_ptr that is not ascending from 0 to n_c ("badptr") must run without touching anything outside the blocks: values unchecked.
No GPU, nothing loaded into Python.  It checks the arithmetic and the bookkeeping of the walk, not the kernels' indexing.

    python tools/ot_segment_host_check.py [--sanitize] [--cxx g++] [--small]

--sanitize builds the program with the address and undefined-behaviour sanitizers (a stand-alone executable with its own main).
--small: the first shapes only."""
import argparse
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np

from tools.ot_host_check import SHIMS, lse_bound, make_case

MAIN = """
static OtLse lse_scan(const float* t, int c0, int c1) {
  OtLse a;
  ot_lse_init(a);
  for (int c = c0; c < c1; ++c) ot_update(a, t[c]);
  return a;
}
// what a lane does with its chunk [c0, c1): rounds of CAND candidates from the chunk's start on, as pair_scan offers them; a round
// inside the current segment (otseg_quiet) without a test per candidate, any other through the walk.  A quiet round may reach past
// the chunk's end, where the kernel's t is -inf and adds nothing.
constexpr int CAND = 4;
static void walk(const float* t, int c0, int c1, const int* seg_ptr, int n_seg, const OtSegOut& o) {
  OtSegWalk w;
  otseg_walk_init(w, seg_ptr);
  for (int j0 = c0; j0 < c1; j0 += CAND) {
    const bool quiet = otseg_quiet(w, j0, CAND);
    for (int j = j0; j < j0 + CAND; ++j) {
      if (quiet) otseg_add(w, j < c1 ? t[j] : -INFINITY);
      else if (j < c1) {
        otseg_advance(w, j, seg_ptr, n_seg, o, true);
        otseg_add(w, t[j]);
      }
    }
  }
  otseg_finish(w, n_seg, o, true);
}

int main(int argc, char** argv) {   // argv: input file, output file
  FILE* f = fopen(argv[1], "rb"); FILE* o = fopen(argv[2], "wb");
  if (!f || !o) return 2;
  int h[5]; float s;   // n_q, n_c, D, n_seg, n_split; s
  if (fread(h, 4, 5, f) != 5 || fread(&s, 4, 1, f) != 1) return 3;
  const int n_q = h[0], n_c = h[1], D = h[2], n_seg = h[3], n_split = h[4];
  std::vector<float> Q((size_t)n_q * D), C((size_t)n_c * D + 1), hv(n_c + 1), t(n_c + 1);
  int* seg_ptr = (int*)malloc(sizeof(int) * (n_seg + 1));   // exactly n_seg + 1 entries: the sanitizer sees a read beyond them
  if (fread(Q.data(), 4, Q.size(), f) != Q.size() || fread(C.data(), 4, (size_t)n_c * D, f) != (size_t)n_c * D || fread(hv.data(), 4, n_c, f) != (size_t)n_c
      || fread(seg_ptr, 4, n_seg + 1, f) != (size_t)n_seg + 1) return 3;
  const size_t nL = (size_t)n_seg * n_q, nW = (size_t)n_split * n_seg * n_q;
  float* L1 = (float*)malloc(4 * nL); float* L2 = (float*)malloc(4 * nL); float* flat = (float*)malloc(4 * (size_t)n_q);
  OtLse* ws = (OtLse*)malloc(sizeof(OtLse) * nW);
  for (size_t e = 0; e < nL; ++e) L1[e] = L2[e] = NAN;
  for (size_t e = 0; e < nW; ++e) ws[e].m = ws[e].sum = NAN;
  const int per = knn_chunk(n_c, n_split);
  if (otseg_ws_bytes(n_q, n_seg, n_split) != (n_split > 1 ? (long long)(nW * sizeof(OtLse)) : 0)) return 5;
  for (int i = 0; i < n_q; ++i) {
    const float* q = Q.data() + (size_t)i * D;
    for (int c = 0; c < n_c; ++c) t[c] = ot_t(knn_d2(q, C.data() + (size_t)c * D, D), s, hv[c]);
    walk(t.data(), 0, n_c, seg_ptr, n_seg, OtSegOut{L1 + i, nullptr, (long)n_q});
    OtLse m;
    ot_lse_init(m);
    for (int c = 0; c < n_split; ++c) {
      const long first = (long)c * per;
      const int c0 = first < n_c ? (int)first : n_c, c1 = first + per < n_c ? (int)(first + per) : n_c;
      walk(t.data(), c0, c1, seg_ptr, n_seg, OtSegOut{nullptr, ws + (size_t)c * n_seg * n_q + i, (long)n_q});
      ot_merge(m, lse_scan(t.data(), c0, c1));
    }
    flat[i] = ot_lse_value(m);
    for (int sg = 0; sg < n_seg; ++sg) L2[(size_t)sg * n_q + i] = otseg_merge(ws + (size_t)sg * n_q + i, (long)n_seg * n_q, n_split);
  }
  for (size_t e = 0; e < nW; ++e) if (ws[e].m != ws[e].m || ws[e].sum != ws[e].sum) return 4;   // a slot no walk wrote
  fwrite(L1, 4, nL, o); fwrite(L2, 4, nL, o); fwrite(flat, 4, n_q, o);
  free(ws); free(flat); free(L2); free(L1); free(seg_ptr);
  fclose(o); fclose(f); return 0;
}
"""
# (n_q, n_c, D, n_seg, n_split, data, s, layout).  Layouts: "even" cuts, "ones" runs of size-1 segments, "empty" empty segments first, last
# and several in a row, "one" a single segment, "badptr" a seg_ptr that is not ascending and runs past n_c
SHAPES = [(5, 40, 3, 4, 3, "lattice", 0.5, "even"), (4, 30, 1, 12, 5, "lattice", 1.0, "empty"), (3, 0, 4, 3, 2, "real", 1.0, "even"),
          (6, 70, 25, 7, 7, "edge", 0.4, "ones"), (5, 50, 10, 1, 4, "real", 0.7, "one"), (4, 60, 5, 6, 3, "real", 0.7, "badptr"),
          (9, 300, 35, 256, 5, "real", 0.3, "ones"), (8, 120, 25, 1, 64, "edge", 2.0, "one"), (4, 257, 64, 2, 2, "real", 0.05, "even"),
          (12, 500, 10, 9, 1, "lattice", 3.0, "empty")]


def host_source() -> str:
    """the three cores as they stand in the headers, between the stand-ins and a main()"""
    def core(name, tag):
        text = open(os.path.join(ROOT, "spvipes_amd", "csrc", name)).read()
        return text[text.index(f"// ---- {tag}-CORE-BEGIN ----"):text.index(f"// ---- {tag}-CORE-END ----")]
    return SHIMS + core("spv_knn.h", "KNN") + core("spv_ot.h", "OT") + core("spv_ot_segments.h", "OTSEG") + MAIN


def make_seg_ptr(rng, n_c, n_seg, layout):
    if layout == "one" or n_seg == 1:
        cuts = np.array([], dtype=np.int64)
    elif layout == "ones":      # size-1 segments from candidate 2 on as long as they last, the rest in the last segment
        cuts = np.minimum(2 + np.arange(n_seg - 1), n_c)
    elif layout == "empty":     # two empty segments first, three in a row in the middle, two last
        inner = np.sort(rng.integers(1, max(n_c, 2), max(n_seg - 8, 0)))
        cuts = np.sort(np.concatenate([[0, 0], inner, [n_c // 2] * 3, [n_c, n_c]]))[:n_seg - 1]
    else:
        cuts = np.sort(rng.integers(0, n_c + 1, n_seg - 1))
    ptr = np.concatenate([[0], cuts, [n_c]]).astype(np.int32)
    if layout == "badptr":
        ptr[1], ptr[2], ptr[-1] = ptr[2] + 5, 1, n_c + 1000
    return ptr


def run(shapes, sanitize=False, cxx="g++", verbose=True) -> int:
    from tests._ot_reference import t_ref
    from tests._ot_segment_reference import segment_lse_ref
    bad = 0
    rng = np.random.default_rng(23)
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "otseg_host.cpp"), os.path.join(d, "otseg_host")
        open(src, "w").write(host_source())
        subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", *(["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []),
                        "-o", exe, src], check=True)
        for n_q, n_c, D, n_seg, n_split, kind, s, layout in shapes:
            Q, C, h = make_case(rng, n_q, n_c, D, kind)
            seg_ptr = make_seg_ptr(rng, n_c, n_seg, layout)
            fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
            with open(fin, "wb") as f:
                f.write(np.array([n_q, n_c, D, n_seg, n_split], np.int32).tobytes() + np.float32(s).tobytes() + Q.tobytes() + C.tobytes() + h.tobytes()
                        + seg_ptr.tobytes())
            subprocess.run([exe, fin, fout], check=True)
            rec = np.fromfile(fout, np.float32)
            L1, L2 = rec[:n_seg * n_q].reshape(n_seg, n_q).T, rec[n_seg * n_q:2 * n_seg * n_q].reshape(n_seg, n_q).T
            flat = rec[2 * n_seg * n_q:]
            ok = [not np.isnan(L1).any() and not np.isnan(L2).any()]
            if layout != "badptr":
                want = segment_lse_ref(t_ref(Q, C, h, s), seg_ptr)
                per = -(-n_c // n_split) if n_c else 0
                for L, nc, ns in ((L1, n_c, 1), (L2, per, n_split)):
                    fin_L = np.isfinite(want)
                    ok.append(bool(np.isneginf(L[~fin_L]).all() and (np.abs(L[fin_L].astype(np.float64) - want[fin_L]) <= lse_bound(want[fin_L], nc, ns, n_c)).all()))
                ok.append(n_seg != 1 or np.array_equal(L2[:, 0].view(np.uint32), flat.view(np.uint32)))
            bad += not all(ok)
            if verbose:
                names = ("all written", "one chunk", "split and merge", "one segment = softmin")
                print(f"n_q {n_q:3d} n_c {n_c:3d} D {D:2d} n_seg {n_seg:3d} n_split {n_split:2d} {kind:8s} {layout:7s} "
                      + "  ".join(f"{n} {'ok' if v else 'DIFFERS'}" for n, v in zip(names, ok)))
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sanitize", action="store_true")
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--cxx", default="g++")
    a = ap.parse_args()
    bad = run(SHAPES[:6] if a.small else SHAPES, a.sanitize, a.cxx)
    print("all within bounds" if not bad else f"{bad} shape(s) DIFFER")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
