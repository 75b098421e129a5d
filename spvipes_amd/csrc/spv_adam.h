// The Adam update as device functions: the bias-correction prologue, the per-element arithmetic and the 16-bit image store.
// adam_kernel, adam_images_kernel (spv_abi.hip) and reduce_adam_fused_kernel (spv_small.h) all go through these, so the three cannot
// drift apart (a different FMA contraction in one of them would already be a different parameter).  torch.optim.Adam semantics.
#pragma once
#include "../../include/spvipes_hip.h"
#include "spv_common.h"

namespace spv {

struct AdamStep { float b1, b2, eps, wd, gscale, step, isq; };

// step = lr / bc1, isq = 1 / sqrt(bc2).  With t_dev the bias corrections 1 - beta^t come from the DEVICE-resident count of completed
// steps (t = *t_dev + 1), in double like torch.optim.Adam's host arithmetic: the launch then carries no per-step host value and can sit
// inside the captured graph of the step.  Nobody writes *t_dev while a kernel that reads it runs (the caller advances it with
// spv_counter_bump after the last of them).  beta^t by repeated squaring.
__device__ __forceinline__ AdamStep adam_prologue(float lr, float b1, float b2, float eps, float wd, float bc1, float bc2, float gscale,
                                                  const long long* t_dev, double b1d, double b2d) {
  if (t_dev) {
    long long e = *t_dev + 1;
    double r1 = 1.0, r2 = 1.0, x1 = b1d, x2 = b2d;
    while (e > 0) { if (e & 1) { r1 *= x1; r2 *= x2; } x1 *= x1; x2 *= x2; e >>= 1; }
    bc1 = (float)(1.0 - r1); bc2 = (float)(1.0 - r2);
  }
  AdamStep a;
  a.b1 = b1; a.b2 = b2; a.eps = eps; a.wd = wd; a.gscale = gscale;
  a.step = lr / bc1; a.isq = rsqrtf(bc2);
  return a;
}

// one element: p, m, v updated in place from the gradient g.  Which product of each sum is fused into it is written out (the forms
// the compiler chose for adam_kernel / adam_images_kernel when the choice was its own): left to the compiler, the same source line
// came out as fma(wd, p, g * gscale) in the kernel that forms g itself and as fma(g, gscale, wd * p) in the two that load it.
__device__ __forceinline__ void adam_update(float& p, float g, float& m, float& v, const AdamStep& a) {
  const float gr = __fmaf_rn(g, a.gscale, __fmul_rn(a.wd, p));                     // g * gscale + wd * p
  m = __fmaf_rn(a.b1, m, __fmul_rn(1.f - a.b1, gr));                              // b1 * m + (1 - b1) * gr
  v = __fmaf_rn(a.b2, v, __fmul_rn(__fmul_rn(1.f - a.b2, gr), gr));               // b2 * v + (1 - b2) * gr * gr
  p -= __fmul_rn(a.step, m) / __fmaf_rn(sqrtf(v), a.isq, a.eps);                  // p - step * m / (sqrt(v) / sqrt(bc2) + eps)
}

// the 16-bit word of an updated value in image q's format
__device__ __forceinline__ uint16_t adam_image_word(const spv_adam_image& q, float x) {
  return q.fmt == SPV_IMAGE_F16 ? f2h(x * q.scale) : f2bf(x);   // (uniform per image: the fc1 weight images are f16 words of W * scale, spv_common.h)
}

// image words of the cnt <= 4 updated values out[0..cnt) whose first element is element k0 >= 0 of image q's parameter (k0 a multiple
// of 4 in the flat kernels; count need not be a multiple of 4): one 8-byte store where the four lie in one row and the address allows
__device__ __forceinline__ void adam_image_store(const spv_adam_image& q, long k0, int cnt, const float (&out)[4]) {
  const unsigned cols = (unsigned)q.cols;
  unsigned r = (unsigned)k0 / cols, c = (unsigned)k0 - r * cols;
  uint16_t* dst = q.dst + ((long)r + q.row_off) * q.ld + q.col_off;
  if (cnt == 4 && k0 + 4 <= q.count && c + 4 <= cols && (((reinterpret_cast<uintptr_t>(dst + c)) & 7) == 0)) {
    typedef __attribute__((ext_vector_type(4))) unsigned short us4;
    *reinterpret_cast<us4*>(dst + c) = us4{adam_image_word(q, out[0]), adam_image_word(q, out[1]), adam_image_word(q, out[2]), adam_image_word(q, out[3])};
  } else {
    for (int j = 0; j < cnt && k0 + j < q.count; ++j) {
      dst[c] = adam_image_word(q, out[j]);
      if (++c == cols) { c = 0; dst += q.ld; }
    }
  }
}

}  // namespace spv
