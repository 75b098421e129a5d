#!/usr/bin/env python3
"""The count sampler on the CPU: compiles `nbmix_draw` (csrc/spv_dec_sample.h) and the Philox helpers (csrc/spv_common.h) as plain C++
with one-line stand-ins for the device intrinsics (libm's expf / logf / exp2f / log2f / cosf, 1 / x, 1 / sqrt(x)), draws the 144-point
grid of tests/_nb_sampling_check.py with it and prints the checker's worst ratios (distribution, mean, variance; each must be <= 1) next
to those of numpy's own samplers.  No GPU.  It checks the algorithm and its fp32 arithmetic, not the device's transcendental units: the
stand-ins are correctly rounded where the hardware instructions are 1 ulp, so the GPU's draws are not bit-identical to these.

    python tools/nbmix_host_check.py [--sanitize] [--key 12345] [--cxx g++]

--sanitize builds the program with the address and undefined-behaviour sanitizers (a stand-alone executable with its own main)."""
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
#define __device__
#define __forceinline__ inline
#define __expf expf
#define __logf logf
static inline float fast_rcp(float x) { return 1.0f / x; }
static inline float rsqrtf(float x) { return 1.0f / sqrtf(x); }
static inline float __builtin_amdgcn_cosf(float x) { return cosf(6.283185307179586f * x); }   // the instruction takes revolutions
static inline float __builtin_amdgcn_exp2f(float x) { return exp2f(x); }
static inline float __builtin_amdgcn_logf(float x) { return log2f(x); }
"""
MAIN = """
int main(int argc, char** argv) {   // argv: grid file ("theta m1 m2 pi" per line), output file (int32), draws per point, key
  FILE* f = fopen(argv[1], "r"); FILE* o = fopen(argv[2], "wb");
  const int n = atoi(argv[3]); const unsigned long long key = strtoull(argv[4], 0, 10);
  if (!f || !o) return 2;
  float th, m1, m2, pi; unsigned g = 0; std::vector<int> buf(n);
  while (fscanf(f, "%f %f %f %f", &th, &m1, &m2, &pi) == 4) {
    const float logit = pi <= 0 ? -INFINITY : pi >= 1 ? INFINITY : logf(pi / (1 - pi));
    for (int r = 0; r < n; ++r) { const NbStream st{{(unsigned)key, (unsigned)(key >> 32)}, g, (unsigned)r, 0u}; buf[r] = nbmix_draw(st, m1, m2, th, logit); }
    fwrite(buf.data(), 4, n, o); ++g;
  }
  fclose(o); return 0;
}
"""


def host_source() -> str:
    """the sampler's device functions as they stand in the headers, between the stand-ins and a main()"""
    csrc = os.path.join(ROOT, "spvipes_amd", "csrc")
    common = open(os.path.join(csrc, "spv_common.h")).read()
    sample = open(os.path.join(csrc, "spv_dec_sample.h")).read()
    philox = common[common.index("__device__ __forceinline__ void philox_round"):common.index("// ---- special functions")]
    body = sample[sample.index("constexpr int NBS_GAMMA_CAP"):sample.index("// ------", sample.index("nbmix_draw(const NbStream"))]
    return SHIMS + philox + body + MAIN


def main():
    from tests import _nb_sampling_check as S
    ap = argparse.ArgumentParser()
    ap.add_argument("--sanitize", action="store_true")
    ap.add_argument("--key", type=int, default=12345)
    ap.add_argument("--cxx", default="g++")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as d:
        src, exe, grid, out = (os.path.join(d, n) for n in ("nbmix_host.cpp", "nbmix_host", "grid.txt", "draws.bin"))
        open(src, "w").write(host_source())
        subprocess.run([a.cxx, "-O2", "-std=c++17", *(["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if a.sanitize else []), "-o", exe, src], check=True)
        open(grid, "w").write("\n".join("%r %r %r %r" % g for g in S.GRID))
        subprocess.run([exe, grid, out, str(S.N_DRAWS), str(a.key)], check=True)
        x = np.fromfile(out, np.int32).reshape(len(S.GRID), S.N_DRAWS)
    rng = np.random.default_rng(0)
    worst, worst_np, bad = np.zeros(3), np.zeros(3), []
    f32 = lambda v: float(np.float32(v))
    for i, (th, m1, m2, pi) in enumerate(S.GRID):
        p = S.pmf_table(f32(m1), f32(m2), f32(th), pi)
        r = S.check(x[i], p)
        worst, worst_np = np.maximum(worst, r), np.maximum(worst_np, S.check(S.numpy_draws(rng, m1, m2, th, pi), p))
        if max(r) > 1.0:
            bad.append(((th, m1, m2, pi), r))
    print("worst ratios, host build of nbmix_draw (distribution, mean, variance):", np.round(worst, 3))
    print("worst ratios, numpy's samplers:                                        ", np.round(worst_np, 3))
    for b in bad:
        print("OUTSIDE THE BOUNDS:", b)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
