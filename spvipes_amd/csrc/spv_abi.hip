// C-ABI entry points of libspvipes_hip.so (see include/spvipes_hip.h).  gfx950 only.
#include "../../include/spvipes_hip.h"
#include "spv_common.h"
#include "spv_gemm.h"
#include "spv_fc1.h"
#include "spv_dec_gemm.h"
#include "spv_decoder.h"
#include "spv_dec_expected.h"
#include "spv_dec_sample.h"
#include "spv_dec_sample_stats.h"
#include "spv_dec_expected_stats.h"
#include "spv_de.h"
#include "spv_de_median.h"
#include "spv_count_stats.h"
#include "spv_knn.h"
#include "spv_ot.h"
#include "spv_ot_segments.h"
#include "spv_ot_project.h"
#include "spv_silhouette.h"
#include "spv_gram.h"
#include "spv_rank.h"
#include "spv_rank_values.h"
#include "spv_pca.h"
#include "spv_tsne.h"
#include "spv_lisi.h"
#include "spv_small.h"
#include "spv_poe_n.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>

using namespace spv;

static thread_local char g_err[512] = "";
static int fail(int code, const char* fmt, const char* what = "") {
  snprintf(g_err, sizeof(g_err), fmt, what);
  return code;
}
static int launch_status(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
    return SPV_ERR_LAUNCH;
  }
  return SPV_OK;
}

// ---- launch idioms the wrappers below share ---------------------------------------------------------------------------------------------
// every pointer on a 16-byte boundary (a null pointer counts as aligned)
template <typename... P>
static bool aligned16(const P*... ptrs) { return ((reinterpret_cast<uintptr_t>(ptrs) | ... | uintptr_t(0)) & 15) == 0; }

static inline int max2(int a, int b) { return a > b ? a : b; }

// launch of kernel K with `bytes` of dynamic LDS (more than the 64 KiB a kernel gets unasked): the one-time opt-in ahead of K's first
// launch, never again (every K has its own flag).  A kernel picked at run time (a `kfn` pointer) sets the attribute per call instead.
template <auto K, typename... Args>
static void launch_lds(dim3 grid, dim3 block, int bytes, hipStream_t s, Args... args) {
  static bool raised = false;
  if (!raised) { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(K), hipFuncAttributeMaxDynamicSharedMemorySize, bytes); raised = true; }
  hipLaunchKernelGGL(K, grid, block, bytes, s, args...);
}
// the same with the opt-in made once to `most`, the largest size any call of K can ask for, and the launch taking `bytes` <= most
template <auto K, typename... Args>
static void launch_lds_upto(dim3 grid, dim3 block, int most, int bytes, hipStream_t s, Args... args) {
  static bool raised = false;
  if (!raised) { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(K), hipFuncAttributeMaxDynamicSharedMemorySize, most); raised = true; }
  hipLaunchKernelGGL(K, grid, block, bytes, s, args...);
}

// The *_grouped entry points: groups go out two at a time while `try_pair(i)` takes groups i and i + 1 as one grid, the rest one by one
// through `run_one(i)` (the per-group entry point).  try_pair returns SPV_OK (launched), NOT_A_PAIR (nothing launched: the two take
// different kernel variants, which ends pairing for this form) or an error code; a second pair form starts where the first one stopped.
static constexpr int NOT_A_PAIR = 1;
template <typename Pair>
static int run_pairs(int& i, int n, Pair try_pair) {
  for (; i + 1 < n; i += 2) {
    const int rc = try_pair(i);
    if (rc == NOT_A_PAIR) break;
    if (rc != SPV_OK) return rc;
  }
  return SPV_OK;
}
template <typename PairA, typename PairB, typename One>
static int pairs_then_rest(int n, PairA try_pair_a, PairB try_pair_b, One run_one) {
  int i = 0;
  int rc = run_pairs(i, n, try_pair_a);
  if (rc == SPV_OK) rc = run_pairs(i, n, try_pair_b);
  for (; rc == SPV_OK && i < n; ++i) rc = run_one(i);
  return rc;
}
template <typename Pair, typename One>
static int pairs_then_rest(int n, Pair try_pair, One run_one) {
  return pairs_then_rest(n, try_pair, [](int) { return NOT_A_PAIR; }, run_one);
}

#ifndef SPV_BUILD_ID
#define SPV_BUILD_ID "00000000000000000000000000000000"
#endif
static const char g_build_id[] = "SPV_BUILD_ID=" SPV_BUILD_ID;   // (the tagged form is also what build.lib_build_id() greps out of the file)
extern "C" int spv_version(void) { return 2; }
extern "C" const char* spv_build_id(void) { return g_build_id + 13; }
extern "C" const char* spv_last_error(void) { return g_err; }

// ---------------------------------------------------------------------------------------------
// pack
// ---------------------------------------------------------------------------------------------
__global__ void pack_bf16_kernel(const float* src, long ld_src, int R, int C, const float* extra_col, int extra_one,
                                 bf16_t* dst_hi, bf16_t* dst_lo, long ld_dst, int dst_col_off, int Rp, int cslot) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long total = (long)Rp * cslot;
  if (idx >= total) return;
  const int r = (int)(idx / cslot), c = (int)(idx % cslot);
  float v = 0.f;
  if (r < R) {
    if (c < C) v = src[(long)r * ld_src + c];
    else if (c == C) v = extra_col ? extra_col[r] : (extra_one ? 1.0f : 0.f);
  }
  bf16_t hi, lo;
  split_bf16(v, hi, lo);
  const long o = (long)r * ld_dst + dst_col_off + c;
  dst_hi[o] = hi;
  if (dst_lo) dst_lo[o] = lo;
}

// 8 consecutive destination columns per thread: one 16-byte store per image
__global__ void pack_bf16_vec8_kernel(const float* src, long ld_src, int R, int C, const float* extra_col, int extra_one,
                                      bf16_t* dst_hi, bf16_t* dst_lo, long ld_dst, int dst_col_off, int Rp, int cslot8) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)Rp * cslot8) return;
  const int r = (int)(idx / cslot8), c0 = (int)(idx % cslot8) * 8;
  unsigned hw[4] = {0u, 0u, 0u, 0u}, lw[4] = {0u, 0u, 0u, 0u};
  if (r < R) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = c0 + j;
      float v = 0.f;
      if (c < C) v = src[(long)r * ld_src + c];
      else if (c == C) v = extra_col ? extra_col[r] : (extra_one ? 1.0f : 0.f);
      bf16_t h, l;
      split_bf16(v, h, l);
      hw[j >> 1] |= (unsigned)h << (16 * (j & 1));
      lw[j >> 1] |= (unsigned)l << (16 * (j & 1));
    }
  }
  const long o = (long)r * ld_dst + dst_col_off + c0;
  *reinterpret_cast<u4v*>(dst_hi + o) = u4v{hw[0], hw[1], hw[2], hw[3]};
  if (dst_lo) *reinterpret_cast<u4v*>(dst_lo + o) = u4v{lw[0], lw[1], lw[2], lw[3]};
}

extern "C" int spv_pack_bf16(const float* src, int64_t ld_src, int32_t R, int32_t C, const float* extra_col,
                             int32_t extra_one, uint16_t* dst_hi, uint16_t* dst_lo, int64_t ld_dst,
                             int32_t dst_col_off, int32_t Rp, int32_t cslot, void* stream) {
  if (!src || !dst_hi || R < 0 || C < 0 || Rp < R || cslot < C + ((extra_col || extra_one) ? 1 : 0) ||
      dst_col_off + cslot > ld_dst)
    return fail(SPV_ERR_ARG, "spv_pack_bf16: bad shape%s");
  const long total = (long)Rp * cslot;
  if (total == 0) return SPV_OK;
  if ((cslot % 8) == 0 && (dst_col_off % 8) == 0 && (ld_dst % 8) == 0 && ((uintptr_t)dst_hi % 16) == 0 && (!dst_lo || ((uintptr_t)dst_lo % 16) == 0)) {
    const long tot8 = total / 8;
    hipLaunchKernelGGL(pack_bf16_vec8_kernel, dim3((unsigned)((tot8 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, src, (long)ld_src, R, C,
                       extra_col, extra_one, dst_hi, dst_lo, (long)ld_dst, dst_col_off, Rp, cslot / 8);
    return launch_status("spv_pack_bf16");
  }
  hipLaunchKernelGGL(pack_bf16_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, src,
                     (long)ld_src, R, C, extra_col, extra_one, dst_hi, dst_lo, (long)ld_dst, dst_col_off, Rp, cslot);
  return launch_status("spv_pack_bf16");
}

// fp32 [R][C] * scale -> IEEE f16 image dst[Rp][ld_dst] (zero filled outside the source): the fc1 weight operand of the
// NSPLIT == 1 mode (spv_common.h).  One thread per 8 destination columns.
__global__ void pack_f16_kernel(const float* src, long ld_src, int R, int C, bf16_t* dst, long ld_dst, int Rp, int cslot8, float scale) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)Rp * cslot8) return;
  const int r = (int)(idx / cslot8), c0 = (int)(idx % cslot8) * 8;
  unsigned w[4] = {0u, 0u, 0u, 0u};
  if (r < R) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = c0 + j;
      const float v = (c < C) ? src[(long)r * ld_src + c] * scale : 0.f;
      w[j >> 1] |= (unsigned)f2h(v) << (16 * (j & 1));
    }
  }
  *reinterpret_cast<u4v*>(dst + (long)r * ld_dst + c0) = u4v{w[0], w[1], w[2], w[3]};
}

extern "C" float spv_fc1_w_scale(void) { return SPV_FC1_W_SCALE; }

extern "C" int spv_pack_f16(const float* src, int64_t ld_src, int32_t R, int32_t C, uint16_t* dst, int64_t ld_dst, int32_t Rp, int32_t cslot,
                            float scale, void* stream) {
  if (!src || !dst || R < 0 || C < 0 || Rp < R || cslot < C || cslot > ld_dst || (cslot % 8) || (ld_dst % 8) || ((uintptr_t)dst % 16))
    return fail(SPV_ERR_ARG, "spv_pack_f16: bad shape (cslot, ld_dst multiples of 8, dst 16-byte aligned)%s");
  const long tot8 = (long)Rp * (cslot / 8);
  if (tot8 == 0) return SPV_OK;
  hipLaunchKernelGGL(pack_f16_kernel, dim3((unsigned)((tot8 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, src, (long)ld_src, R, C, dst, (long)ld_dst,
                     Rp, cslot / 8, scale);
  return launch_status("spv_pack_f16");
}

// ---------------------------------------------------------------------------------------------
// encoder fc1
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void fc1_epilogue_body(const float* slabs, const float* rowsum_ws, int splits, int B, int N1, const float* bias,
                                                  const float* bias2, int n_first, float* h1, float* library, const float* library_all,
                                                  const int* rows, float acc_scale, const float* cov, const int* cov_idx) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long total = (long)B * N1;
  if (idx < total) {
    const int col = (int)(idx % N1);
    const float bv = (bias2 != nullptr && col >= n_first) ? bias2[col - n_first] : bias[col];
    const float cv = cov ? cov[(long)cov_idx[idx / N1] * N1 + col] : 0.f;   // one-hot batch covariates (nn/networks.py:105-119): a per-cell bias row
    float v = 0.f;
    for (int s = 0; s < splits; ++s) v += slabs[(long)s * total + idx];
    h1[idx] = fmaxf(v * acc_scale + bv + cv, 0.f);  // relu(fc1(x)), nn/networks.py:119
  }
  if (idx < B) {
    if (library_all != nullptr) {  // precomputed per cell of the data set (spv_prepare_log1p)
      library[idx] = library_all[rows ? rows[idx] : (int)idx];
    } else {
      float v = 0.f;
      for (int s = 0; s < splits; ++s) v += rowsum_ws[(long)s * B + idx];
      library[idx] = __logf(v);  // log(sum of log1p(x)), module/spVIPESmodule.py:435
    }
  }
}
__global__ void fc1_epilogue_kernel(const float* slabs, const float* rowsum_ws, int splits, int B, int N1, const float* bias,
                                    const float* bias2, int n_first, float* h1, float* library, const float* library_all,
                                    const int* rows, float acc_scale, const float* cov, const int* cov_idx) {
  fc1_epilogue_body(slabs, rowsum_ws, splits, B, N1, bias, bias2, n_first, h1, library, library_all, rows, acc_scale, cov, cov_idx);
}

struct Fc1EpiPlainArgs { const float* slabs; const float* rowsum_ws; int splits, B, N1; const float* bias; const float* bias2; int n_first; float* h1; float* library;
                         const float* library_all; const int* rows; float acc_scale; const float* cov; const int* cov_idx; };
__global__ void fc1_epilogue_pair_kernel(Fc1EpiPlainArgs a0, Fc1EpiPlainArgs a1) {   // blockIdx.y = group
  const Fc1EpiPlainArgs a = blockIdx.y ? a1 : a0;
  fc1_epilogue_body(a.slabs, a.rowsum_ws, a.splits, a.B, a.N1, a.bias, a.bias2, a.n_first, a.h1, a.library, a.library_all, a.rows, a.acc_scale, a.cov, a.cov_idx);
}

// every 8-gene chunk of a row is one aligned 16-byte load when base, row pitch and column offset are
static int counts_aligned(const spv_counts* x) {
  const long esz = (x->dtype == SPV_COUNT_U16) ? 2 : 4;
  return ((reinterpret_cast<uintptr_t>(x->X) & 15) == 0) && ((x->ld * esz) % 16 == 0) && ((x->col_off * esz) % 16 == 0);
}

template <typename CT, int NSPLIT>
static int fc1_fwd_dispatch(const GemmParams& p, int N1, int splits, hipStream_t s) {
  constexpr bool HF = NSPLIT == 1;   // 16-bit operand words of the one-MFMA mode are f16 (spv_common.h)
  if (N1 <= 32) return launch_gemm<GemmCfg<128, 32, 4, 1, false, false, SRC_COUNTS, SRC_PLAIN, CT, NSPLIT, 32, 4, 1, HF>>(p, splits, s);
  if (N1 <= 128) return launch_gemm<GemmCfg<64, 128, 2, 2, false, false, SRC_COUNTS, SRC_PLAIN, CT, NSPLIT, 32, 4, 1, HF>>(p, splits, s);
  if constexpr (NSPLIT == 1) {
    if (p.M >= 1024) return launch_gemm<GemmCfg<128, 256, 2, 2, false, false, SRC_COUNTS, SRC_PLAIN, CT, NSPLIT, 32, 2, 2, HF>>(p, splits, s);  // 64 x 128 wave tiles
  }
  return launch_gemm<GemmCfg<64, 256, 1, 4, false, false, SRC_COUNTS, SRC_PLAIN, CT, NSPLIT, 32, 4, 1, HF>>(p, splits, s);
}

// Shapes the LDS-DMA fc1 forward kernel (spv_fc1.h) takes: the resident bf16 log1p image, both encoders' 2H = 256 output columns,
// operand images zero padded to multiples of 64 genes with 16-byte aligned rows.  The host asks through this entry point
// because the path fixes the slab workspace: [splits][round_up(B, 128)][256] fp32 in accumulator-tile order.
extern "C" int spv_enc_fc1_fwd_uses_dma(int32_t B, int32_t G, int32_t N1, int32_t nsplit, int32_t have_xb, int64_t ldw, int64_t ld_xb) {
  const long G64 = (G + 63) & ~63L;
  if (nsplit == 3)   // "fp32" mode: the resident image holds [hi | lo] halves per row (spv_prepare_log1p_split): ld_xb is the pitch of both
    return have_xb && (N1 == F1_BN || N1 == 2 * F1_BN) && B > 0 && G > 0 && ldw >= G64 && ld_xb >= 2 * G64 && (ldw % 8) == 0 && (ld_xb % 16) == 0;
  return have_xb && nsplit == 1 && (N1 == F1_BN || N1 == 2 * F1_BN) && B > 0 && G > 0 && ldw >= G64 && ld_xb >= G64 && (ldw % 8) == 0 && (ld_xb % 8) == 0;
}

static int fc1_bn(int N1) { return N1 <= 32 ? 32 : (N1 <= 128 ? 128 : 256); }

// operands of the fc1 forward GEMM, `bk`-deep k steps: the counts themselves (decoded by the kernel, which also sums the rows), or --
// xb_all -- the resident log1p image of the data set (spv_prepare_log1p): a plain gathered operand, no decode
// (nsplit 3: hi / lo planes interleaved inside the image rows, spv_prepare_log1p_split)
static GemmParams fc1_fwd_params(const spv_fc1_fwd_args& a, int bk) {
  GemmParams p{};
  p.A = a.x->X; p.A_lo = nullptr; p.lda = a.x->ld;
  p.B = a.W1_hi; p.B_lo = a.W1_lo; p.ldb = a.ldw;
  p.rows = a.x->rows; p.counts_aligned = counts_aligned(a.x); p.col_off = a.x->col_off; p.n_cells = a.B; p.n_genes = a.G;
  p.rowsum = a.rowsum_ws;
  if (a.xb_all != nullptr) { p.A = a.xb_all; p.lda = a.ld_xb; p.rowsum = nullptr; }
  p.C = a.slabs; p.ldc = a.N1; p.slab_stride = (long)a.B * a.N1;
  p.M = a.B; p.N = a.N1; p.K = a.G;
  const int ktiles = (a.G + bk - 1) / bk;
  p.k_per_split = ((ktiles + a.splits - 1) / a.splits) * bk;
  p.epi = EPI_STORE;
  return p;
}

extern "C" int spv_enc_fc1_fwd(const spv_counts* x, int32_t B, int32_t G, const uint16_t* W1_hi, const uint16_t* W1_lo,
                               int64_t ldw, int32_t N1, const float* bias, const float* bias2, int32_t n_first, int32_t nsplit,
                               int32_t splits, float* slabs, float* rowsum_ws, float* h1, float* library, const uint16_t* xb_all,
                               int64_t ld_xb, const float* library_all, const float* cov, const int32_t* cov_idx, void* stream) {
  if (!x || !x->X || !W1_hi || !bias || !slabs || !rowsum_ws || !h1 || !library) return fail(SPV_ERR_ARG, "spv_enc_fc1_fwd: null pointer%s");
  if ((cov == nullptr) != (cov_idx == nullptr)) return fail(SPV_ERR_ARG, "spv_enc_fc1_fwd: cov and cov_idx go together%s");
  if (B <= 0 || G <= 0 || N1 <= 0 || splits <= 0 || (ldw % 32) != 0 || ldw < ((G + 31) & ~31)) return fail(SPV_ERR_ARG, "spv_enc_fc1_fwd: bad shape%s");
  if (nsplit != 1 && nsplit != 3) return fail(SPV_ERR_ARG, "spv_enc_fc1_fwd: nsplit must be 1 or 3%s");
  if (nsplit == 3 && !W1_lo) return fail(SPV_ERR_ARG, "spv_enc_fc1_fwd: nsplit=3 needs W1_lo%s");
  if (xb_all != nullptr) {
    if (!library_all || ld_xb < ((G + 31) & ~31) || (ld_xb % 8)) return fail(SPV_ERR_ARG, "spv_enc_fc1_fwd: xb_all needs library_all and ld_xb >= round_up(G, 32)%s");
    if (nsplit == 3 && !spv_enc_fc1_fwd_uses_dma(B, G, N1, nsplit, 1, ldw, ld_xb)) return fail(SPV_ERR_ARG, "spv_enc_fc1_fwd: a split (nsplit 3) resident image is only taken by the LDS-DMA kernel (ask spv_enc_fc1_fwd_uses_dma)%s");
  }
  // resident-image path with both encoders' 2H > 128 columns: 128 x 256 tiles, 64-deep k steps and ONE register stage
  // (the 64 x 128 wave tile holds 128 accumulator registers; a deeper prefetch ring spills at two workgroups per CU --
  // measured 88 -> 62 us) when both images are zero padded to a multiple of 64 genes, else 32-deep steps
  const int G64 = (G + 63) & ~63;
  const bool wide64 = xb_all != nullptr && N1 > 128 && ld_xb >= G64 && ldw >= G64;
  const spv_fc1_fwd_args a{x, B, G, W1_hi, W1_lo, ldw, N1, bias, bias2, n_first, nsplit, splits, slabs, rowsum_ws, h1, library, xb_all, ld_xb, library_all, cov, cov_idx};
  GemmParams p = fc1_fwd_params(a, wide64 ? 64 : 32);
  hipStream_t s = (hipStream_t)stream;
  int rc;
  const float acc_scale = (nsplit == 1) ? 1.0f / SPV_FC1_W_SCALE : 1.0f;   // the f16 weight image holds W * SPV_FC1_W_SCALE (spv_pack_f16)
  if (spv_enc_fc1_fwd_uses_dma(B, G, N1, nsplit, xb_all != nullptr, ldw, ld_xb)) {
    // LDS-DMA kernel (spv_fc1.h): 128-cell tiles, K split `splits` ways, slabs in accumulator-tile order [splits][Mp128][256].
    // "fp32" mode on a resident split image: the same kernel on hi / lo planes (fc1_fwd_dma_body<true>), which is that image's only
    // consumer (checked above); a misaligned 16-bit image goes to the register-staged kernels below
    const bool split = nsplit == 3, aligned = aligned16(xb_all, W1_hi, split ? W1_lo : nullptr);
    if (split && !aligned) return fail(SPV_ERR_ARG, "spv_enc_fc1_fwd: images must be 16-byte aligned%s");
    if (aligned) {
      const int mtiles = (B + F1_BM - 1) / F1_BM, kt = (G + F1_BK - 1) / F1_BK;
      p.k_per_split = ((kt + splits - 1) / splits) * F1_BK;
      p.c_split_row = splits;
      const dim3 grid(mtiles * splits, N1 / F1_BN);
      if (split) launch_lds<fc1_fwd_dma_split_kernel>(grid, dim3(512), F1_LDS_BYTES, s, p);
      else launch_lds<fc1_fwd_dma_kernel>(grid, dim3(512), F1_LDS_BYTES, s, p);
      if ((rc = launch_status(split ? "spv_enc_fc1_fwd dma split gemm" : "spv_enc_fc1_fwd dma gemm")) != SPV_OK) return rc;
      const long slab_elems = (long)mtiles * F1_BM * N1;
      hipLaunchKernelGGL(fc1_epilogue_tiled_kernel, dim3((unsigned)((slab_elems / 4 + 255) / 256)), dim3(256), 0, s, slabs, splits, slab_elems, B, N1, bias, bias2, n_first, h1, library,
                         library_all, x->rows, acc_scale, cov, cov_idx);
      return launch_status(split ? "spv_enc_fc1_fwd dma split epilogue" : "spv_enc_fc1_fwd dma epilogue");
    }
  }
  if (xb_all != nullptr) {
    if (N1 <= 128) rc = launch_gemm<GemmCfg<64, 128, 2, 2, false, false, SRC_GATHER, SRC_PLAIN, unsigned short, 1, 32, 4, 1, true>>(p, splits, s);
    else if (wide64) rc = launch_gemm<GemmCfg<128, 256, 2, 2, false, false, SRC_GATHER, SRC_PLAIN, unsigned short, 1, 64, 1, 2, true>>(p, splits, s);
    else rc = launch_gemm<GemmCfg<128, 256, 2, 2, false, false, SRC_GATHER, SRC_PLAIN, unsigned short, 1, 32, 2, 2, true>>(p, splits, s);
  } else if (x->dtype == SPV_COUNT_U16) rc = (nsplit == 3) ? fc1_fwd_dispatch<unsigned short, 3>(p, N1, splits, s) : fc1_fwd_dispatch<unsigned short, 1>(p, N1, splits, s);
  else if (x->dtype == SPV_COUNT_F32) rc = (nsplit == 3) ? fc1_fwd_dispatch<float, 3>(p, N1, splits, s) : fc1_fwd_dispatch<float, 1>(p, N1, splits, s);
  else return fail(SPV_ERR_ARG, "spv_enc_fc1_fwd: unknown count dtype%s");
  if (rc != SPV_OK) return launch_status("spv_enc_fc1_fwd gemm");
  const long total = (long)B * N1;
  hipLaunchKernelGGL(fc1_epilogue_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, slabs, rowsum_ws, splits, B, N1, bias, bias2, n_first, h1, library, xb_all ? library_all : nullptr, x->rows, acc_scale, cov, cov_idx);
  return launch_status("spv_enc_fc1_fwd epilogue");
}

// 1 when spv_enc_fc1_wgrad takes a split (nsplit 3) resident image for these shapes (the LDS-DMA kernel is its only consumer)
extern "C" int spv_enc_fc1_wgrad_split_uses_dma(int32_t B, int32_t G, int32_t N1, int64_t ld_dh, int64_t ld_xb) {
  if (B <= 0 || G <= 0) return 0;
  const int Kpad = (B + FW_BK - 1) / FW_BK * FW_BK;
  return (N1 == FW_BM || N1 == 2 * FW_BM) && ld_dh == N1 && ld_xb >= 2 * (((long)G + 95) / 96 * 96) && (ld_xb % 128) == 0 && fw_lds_bytes(96, Kpad) <= 160 * 1024;
}

// operands of the fc1 weight-gradient GEMM (the arguments of spv_enc_fc1_wgrad): dh image x the counts, or -- xb -- x the resident
// log1p image of the data set: a gathered plain k-major operand, no decode
static GemmParams fc1_wgrad_params(const spv_counts* x, int B, int G, const uint16_t* dh_hi, const uint16_t* dh_lo, long ld_dh, int N1, int nsplit, float* dW,
                                   float* dW2, int rows_first, long ldc, const uint16_t* xb, long ld_xb, const float* dh_scale) {
  GemmParams p{};
  p.A = dh_hi; p.A_lo = dh_lo; p.lda = ld_dh;
  p.B = x->X; p.B_lo = nullptr; p.ldb = x->ld;
  if (xb != nullptr) { p.B = xb; p.ldb = ld_xb; }
  p.rows = x->rows; p.counts_aligned = counts_aligned(x); p.col_off = x->col_off; p.n_cells = B; p.n_genes = G;
  p.rowsum = nullptr;
  p.C = dW; p.ldc = ldc; p.slab_stride = 0;
  p.C2 = dW2; p.c_split_row = rows_first;
  p.out_scale = (nsplit == 1) ? dh_scale + 1 : nullptr;   // {scale, 1 / scale} of the f16 dh image
  p.M = N1; p.N = G; p.K = B;
  p.k_per_split = (B + 63) & ~63;
  p.epi = EPI_STORE;
  return p;
}

extern "C" int spv_enc_fc1_wgrad(const spv_counts* x, int32_t B, int32_t G, const uint16_t* dh_hi, const uint16_t* dh_lo,
                                 int64_t ld_dh, int32_t N1, int32_t nsplit, float* dW, float* dW2, int32_t rows_first, int64_t ldc,
                                 const uint16_t* xb, int64_t ld_xb, const float* dh_scale, void* stream) {
  if (!x || !x->X || !dh_hi || !dW) return fail(SPV_ERR_ARG, "spv_enc_fc1_wgrad: null pointer%s");
  if (nsplit == 1 && !dh_scale) return fail(SPV_ERR_ARG, "spv_enc_fc1_wgrad: nsplit=1 needs the dh image's scale record (spv_enc_fc1_bwd_prep)%s");
  if (B <= 0 || G <= 0 || N1 <= 0 || ld_dh < ((N1 + 127) & ~127) || (ld_dh % 8) != 0 || ldc < G) return fail(SPV_ERR_ARG, "spv_enc_fc1_wgrad: bad shape%s");
  if (nsplit != 1 && nsplit != 3) return fail(SPV_ERR_ARG, "spv_enc_fc1_wgrad: nsplit must be 1 or 3%s");
  if (nsplit == 3 && !dh_lo) return fail(SPV_ERR_ARG, "spv_enc_fc1_wgrad: nsplit=3 needs dh_lo%s");
  const GemmParams p = fc1_wgrad_params(x, B, G, dh_hi, dh_lo, ld_dh, N1, nsplit, dW, dW2, rows_first, ldc, xb, ld_xb, dh_scale);
  hipStream_t s = (hipStream_t)stream;
  int rc;
  if (xb != nullptr && nsplit == 3) {
    // "fp32" mode on the resident split image (spv_prepare_log1p_split): the LDS-DMA kernel on hi / lo planes, 96-gene tiles
    const int Kpad = (B + FW_BK - 1) / FW_BK * FW_BK;
    if (!spv_enc_fc1_wgrad_split_uses_dma(B, G, N1, ld_dh, ld_xb) || rows_first != N1 / 2 || dW2 == nullptr || !aligned16(xb, dh_hi, dh_lo))
      return fail(SPV_ERR_ARG, "spv_enc_fc1_wgrad: a split (nsplit 3) resident image is only taken by the LDS-DMA kernel (ask spv_enc_fc1_wgrad_split_uses_dma)%s");
    // gene tile: 128 where that saves a round of one-per-CU workgroups over 96 (and its LDS need -- 144 KiB of stages + the row table -- fits)
    const int mth = N1 / FW_BM, nb96 = (G + 95) / 96, nb128 = (G + 127) / 128;
    const bool fits128 = fw_lds_bytes(128, Kpad) <= 160 * 1024 && ld_xb >= 2 * (long)nb128 * 128;
    const bool use128 = fits128 && (nb128 * mth + 255) / 256 < (nb96 * mth + 255) / 256;
    void (*kfn)(GemmParams) = use128 ? fc1_wgrad_dma_split_kernel<128> : fc1_wgrad_dma_split_kernel<96>;
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    hipLaunchKernelGGL(kfn, dim3(use128 ? nb128 : nb96, mth), dim3(512), fw_lds_bytes(use128 ? 128 : 96, Kpad), s, p);
    return launch_status("spv_enc_fc1_wgrad dma split");
  }
  if (xb != nullptr) {
    if (nsplit != 1 || ld_xb < ((G + 63) & ~63) || (ld_xb % 8)) return fail(SPV_ERR_ARG, "spv_enc_fc1_wgrad: xb needs nsplit 1 and ld_xb >= round_up(G, 64)%s");
    const int Kpad = (B + FW_BK - 1) / FW_BK * FW_BK;
    if ((N1 == FW_BM || N1 == 2 * FW_BM) && ld_dh == N1 && rows_first == N1 / 2 && dW2 != nullptr && fw_lds_bytes(64, Kpad) <= 160 * 1024 && aligned16(xb, dh_hi)) {
      // LDS-DMA kernel (spv_fc1.h): all 256 rows x 64 genes per workgroup over the whole batch, results straight into dW / dW2
      // (measured at C2, tools/probes/fc1w_bench.hip: 51 us alone against 75 us for the register-staged kernel below)
      // 96-gene tiles when they put TWO groups' launches (two streams, one workgroup per CU) into one round of the 256 CUs and
      // 64-gene tiles do not (C2: 2 x 105 against 2 x 157 workgroups; alone the 64-gene tile is the faster one)
      const int nb64 = (G + 63) / 64, nb96 = (G + 95) / 96;
      const bool use96 = 2 * nb96 <= 256 && 2 * nb64 > 256 && fw_lds_bytes(96, Kpad) <= 160 * 1024;
      void (*kfn)(GemmParams) = use96 ? fc1_wgrad_dma_kernel<96> : fc1_wgrad_dma_kernel<64>;
      const int lds = fw_lds_bytes(use96 ? 96 : 64, Kpad);
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
      hipLaunchKernelGGL(kfn, dim3(use96 ? nb96 : nb64, N1 / FW_BM), dim3(512), lds, s, p);
      return launch_status("spv_enc_fc1_wgrad dma");
    }
    // 96-gene tiles when the image rows are padded that far: at G = 10 000 that is 2 x 105 workgroups per group, so the two
    // groups' GEMMs (two streams) are resident together in one round instead of 2 x 314 workgroups in two (-0.04 ms per
    // step; alone the 64-gene tile is 4 us faster)
    if (ld_xb >= (G + 95) / 96 * 96) rc = launch_gemm<GemmCfg<128, 96, 4, 1, true, true, SRC_PLAIN, SRC_GATHER, unsigned short, 1, 64, 4, 1, true>>(p, 1, s);
    else rc = launch_gemm<GemmCfg<128, 64, 4, 1, true, true, SRC_PLAIN, SRC_GATHER, unsigned short, 1, 64, 4, 1, true>>(p, 1, s);
  } else if (x->dtype == SPV_COUNT_U16) {
    rc = (nsplit == 3) ? launch_gemm<GemmCfg<128, 64, 4, 1, true, true, SRC_PLAIN, SRC_COUNTS, unsigned short, 3, 64, 4>>(p, 1, s)
                       : launch_gemm<GemmCfg<128, 64, 4, 1, true, true, SRC_PLAIN, SRC_COUNTS, unsigned short, 1, 64, 4, 1, true>>(p, 1, s);
  } else if (x->dtype == SPV_COUNT_F32) {
    rc = (nsplit == 3) ? launch_gemm<GemmCfg<128, 64, 4, 1, true, true, SRC_PLAIN, SRC_COUNTS, float, 3, 64, 4>>(p, 1, s)
                       : launch_gemm<GemmCfg<128, 64, 4, 1, true, true, SRC_PLAIN, SRC_COUNTS, float, 1, 64, 4, 1, true>>(p, 1, s);
  } else return fail(SPV_ERR_ARG, "spv_enc_fc1_wgrad: unknown count dtype%s");
  (void)rc;
  return launch_status("spv_enc_fc1_wgrad");
}


// ---------------------------------------------------------------------------------------------
template <bool A_KMAJ, int NSPLIT, int A_SRC>
static int gemm_dispatch(const GemmParams& p, int splits, hipStream_t s) {
  if (p.N <= 32) return launch_gemm<GemmCfg<128, 32, 4, 1, A_KMAJ, true, A_SRC, SRC_PLAIN, unsigned short, NSPLIT, 64, 4>>(p, splits, s);
  return launch_gemm<GemmCfg<64, 320, 2, 2, A_KMAJ, true, A_SRC, SRC_PLAIN, unsigned short, NSPLIT, 64, 1, (NSPLIT == 1 ? 2 : 1)>>(p, splits, s);
}

// Shapes the LDS-DMA 320-column kernels (spv_dec_gemm.h) take: bf16 mode, a tile-ordered [cells][genes] A operand, a 320-wide
// k-major B image.  The tiled array must cover round_up(M, 128) x round_up(K, 64) (cells x genes, a_kmajor 0) or
// round_up(K, 64) x round_up(M, 128) (a_kmajor 1): the decoder's Bp / Gp paddings (multiples of 128 / 256) do.
extern "C" int spv_gemm_bf16_uses_dma(int32_t a_kmajor, int32_t M, int32_t N, int32_t K, int32_t nsplit, int32_t a_tiles, int64_t ldb) {
  if ((nsplit != 1 && nsplit != 3) || a_tiles <= 0 || N <= 32 || N > DG_BN || ldb != DG_BN || M <= 0 || K <= 0) return 0;
  const long genes_needed = a_kmajor ? ((long)M + DG_BM - 1) / DG_BM * DG_BM : ((long)K + DG_BK - 1) / DG_BK * DG_BK;
  if ((long)a_tiles * 32 < genes_needed) return 0;
  return 1;
}

extern "C" int spv_gemm_bf16(int32_t a_kmajor, const uint16_t* A_hi, const uint16_t* A_lo, int64_t lda, const uint16_t* B_hi,
                             const uint16_t* B_lo, int64_t ldb, float* C, int64_t ldc, int32_t M, int32_t N, int32_t K,
                             int32_t nsplit, int32_t splits, int64_t slab_stride, int32_t a_tiles, void* stream) {
  return spv_gemm_bf16_fix(a_kmajor, A_hi, A_lo, lda, B_hi, B_lo, ldb, C, ldc, M, N, K, nsplit, splits, slab_stride, a_tiles, nullptr, stream);
}

extern "C" int spv_gemm_bf16_fix(int32_t a_kmajor, const uint16_t* A_hi, const uint16_t* A_lo, int64_t lda, const uint16_t* B_hi,
                                 const uint16_t* B_lo, int64_t ldb, float* C, int64_t ldc, int32_t M, int32_t N, int32_t K,
                                 int32_t nsplit, int32_t splits, int64_t slab_stride, int32_t a_tiles, const spv_gemm_fixup* fix, void* stream) {
  if (!A_hi || !B_hi || !C) return fail(SPV_ERR_ARG, "spv_gemm_bf16: null pointer%s");
  if (fix) {
    if (!spv_gemm_bf16_uses_dma(a_kmajor, M, N, K, nsplit, a_tiles, ldb)) return fail(SPV_ERR_UNSUPPORTED, "spv_gemm_bf16_fix: only the LDS-DMA 320-column kernels sum their slabs in the launch%s");
    if (!fix->counters || !fix->dst0 || fix->n0 <= 0 || fix->n0 > N || fix->ld0 < fix->n0 || (ldc & 3) || (slab_stride & 3) || !aligned16(C) ||
        (fix->dst1 && (fix->c1 < fix->n0 || fix->n1 <= 0 || fix->c1 + fix->n1 > N || fix->ld1 < fix->n1)) || ldc < N)
      return fail(SPV_ERR_ARG, "spv_gemm_bf16_fix: bad fix-up description%s");
    // (the LDS-DMA kernels want 16-byte aligned planes; the register-staged kernels they would fall back to know nothing of the fix-up)
    if (!aligned16(A_hi, B_hi) || (nsplit == 3 && !aligned16(A_lo, B_lo)))
      return fail(SPV_ERR_ARG, "spv_gemm_bf16_fix: operand planes must be 16-byte aligned%s");
  }
  if (M <= 0 || N <= 0 || K <= 0 || splits <= 0 || (!a_tiles && (lda % 8)) || (ldb % 8) || a_tiles < 0) return fail(SPV_ERR_ARG, "spv_gemm_bf16: bad shape%s");
  if (nsplit != 1 && nsplit != 3) return fail(SPV_ERR_ARG, "spv_gemm_bf16: nsplit must be 1 or 3%s");
  if (nsplit == 3 && (!A_lo || !B_lo)) return fail(SPV_ERR_ARG, "spv_gemm_bf16: nsplit=3 needs lo images%s");
  const int bn = (N <= 32) ? 32 : 320;
  if (ldb < ((N + bn - 1) / bn) * bn) return fail(SPV_ERR_ARG, "spv_gemm_bf16: B image narrower than the N tiling%s");
  GemmParams p{};
  p.A = A_hi; p.A_lo = A_lo; p.lda = lda;
  p.B = B_hi; p.B_lo = B_lo; p.ldb = ldb;
  p.C = C; p.ldc = ldc; p.slab_stride = slab_stride;
  p.M = M; p.N = N; p.K = K;
  const int ktiles = (K + 63) / 64;  // BK = 64: operands are padded to multiples of 64 along K
  p.k_per_split = ((ktiles + splits - 1) / splits) * 64;
  p.epi = EPI_STORE;
  p.tiles_inner = a_tiles;
  if (fix) {
    p.fix_cnt = fix->counters; p.fix_alpha = fix->alpha; p.fix_d0 = fix->dst0; p.fix_ld0 = fix->ld0; p.fix_n0 = fix->n0;
    p.fix_d1 = fix->dst1; p.fix_ld1 = fix->ld1; p.fix_c1 = fix->c1; p.fix_n1 = fix->n1;
  }
  hipStream_t s = (hipStream_t)stream;
  if (nsplit == 3 && spv_gemm_bf16_uses_dma(a_kmajor, M, N, K, nsplit, a_tiles, ldb) && aligned16(A_hi, B_hi, A_lo, B_lo)) {
    // split-bf16 operands ("fp32" mode): the same tiles from hi and lo planes, 16-deep stages, three MFMAs per fragment pair
    const int mtiles = (M + DG_BM - 1) / DG_BM;
    p.c_split_row = splits;
    if (a_kmajor) launch_lds<dec_gemm320_dma4s_kernel<true>>(dim3(mtiles * splits), dim3(512), D4S_LDS_BYTES, s, p);
    else launch_lds<dec_gemm320_dma4s_kernel<false>>(dim3(mtiles * splits), dim3(512), D4S_LDS_BYTES, s, p);
    return launch_status("spv_gemm_bf16 dma split");
  }
  if (nsplit == 1 && spv_gemm_bf16_uses_dma(a_kmajor, M, N, K, nsplit, a_tiles, ldb) && aligned16(A_hi, B_hi)) {
    // LDS-DMA kernels (spv_dec_gemm.h): 128 x 320 workgroup tiles, `splits` K ranges, four 28 KiB stages (measured at C2,
    // tools/probes/dec_gemm_bench.hip: d A_m 37.5 us, d W_m 38.9 us against 76.5 / 84.8 us for the register-staged 64 x 320 kernel below;
    // the two-stage x 64-deep version of the same kernel: 38.2 / 41.5 us)
    const int mtiles = (M + DG_BM - 1) / DG_BM;
    p.c_split_row = splits;
    if (a_kmajor) launch_lds<dec_gemm320_dma4_kernel<true>>(dim3(mtiles * splits), dim3(512), D4_LDS_BYTES, s, p);
    else launch_lds<dec_gemm320_dma4_kernel<false>>(dim3(mtiles * splits), dim3(512), D4_LDS_BYTES, s, p);
    return launch_status("spv_gemm_bf16 dma");
  }
  if (a_tiles) {
    if (a_kmajor) { if (nsplit == 3) gemm_dispatch<true, 3, SRC_TILED>(p, splits, s); else gemm_dispatch<true, 1, SRC_TILED>(p, splits, s); }
    else { if (nsplit == 3) gemm_dispatch<false, 3, SRC_TILED>(p, splits, s); else gemm_dispatch<false, 1, SRC_TILED>(p, splits, s); }
  } else {
    if (a_kmajor) { if (nsplit == 3) gemm_dispatch<true, 3, SRC_PLAIN>(p, splits, s); else gemm_dispatch<true, 1, SRC_PLAIN>(p, splits, s); }
    else { if (nsplit == 3) gemm_dispatch<false, 3, SRC_PLAIN>(p, splits, s); else gemm_dispatch<false, 1, SRC_PLAIN>(p, splits, s); }
  }
  return launch_status("spv_gemm_bf16");
}

// both groups' 320-column GEMMs of the decoder backward (same direction, bf16 words, LDS-DMA shapes) as one grid; anything else: per group
static bool gemm_pair_ok(const spv_gemm_args& a) {
  return a.A_hi && a.B_hi && a.C && a.nsplit == 1 && a.M > 0 && a.N > 0 && a.K > 0 && a.splits > 0 &&
         spv_gemm_bf16_uses_dma(a.a_kmajor, a.M, a.N, a.K, a.nsplit, a.a_tiles, a.ldb) && aligned16(a.A_hi, a.B_hi);
}
static GemmParams gemm_pair_params(const spv_gemm_args& a) {
  GemmParams p{};
  p.A = a.A_hi; p.lda = a.lda; p.B = a.B_hi; p.ldb = a.ldb; p.C = a.C; p.ldc = a.ldc; p.slab_stride = a.slab_stride;
  p.M = a.M; p.N = a.N; p.K = a.K;
  const int ktiles = (a.K + 63) / 64;
  p.k_per_split = ((ktiles + a.splits - 1) / a.splits) * 64;
  p.epi = EPI_STORE; p.tiles_inner = a.a_tiles; p.c_split_row = a.splits;
  return p;
}
extern "C" int spv_gemm_bf16_grouped(const spv_gemm_args* g, int32_t n, void* stream) {
  if (!g || n <= 0) return fail(SPV_ERR_ARG, "spv_gemm_bf16_grouped: bad arguments%s");
  hipStream_t s = (hipStream_t)stream;
  return pairs_then_rest(n,
    [&](int i) {
      const spv_gemm_args &a = g[i], &b = g[i + 1];
      if (!(gemm_pair_ok(a) && gemm_pair_ok(b) && a.a_kmajor == b.a_kmajor)) return NOT_A_PAIR;
      const GemmParams p0 = gemm_pair_params(a), p1 = gemm_pair_params(b);
      const int n0 = (a.M + DG_BM - 1) / DG_BM * a.splits, n1 = (b.M + DG_BM - 1) / DG_BM * b.splits;
      if (a.a_kmajor) launch_lds<dec_gemm320_dma4_pair_kernel<true>>(dim3(max2(n0, n1), 2), dim3(512), D4_LDS_BYTES, s, p0, p1);
      else launch_lds<dec_gemm320_dma4_pair_kernel<false>>(dim3(max2(n0, n1), 2), dim3(512), D4_LDS_BYTES, s, p0, p1);
      return launch_status("spv_gemm_bf16_grouped");
    },
    [&](int i) {
      const spv_gemm_args& a = g[i];
      return spv_gemm_bf16(a.a_kmajor, a.A_hi, a.A_lo, a.lda, a.B_hi, a.B_lo, a.ldb, a.C, a.ldc, a.M, a.N, a.K, a.nsplit, a.splits, a.slab_stride, a.a_tiles, stream);
    });
}

extern "C" int spv_dec_heads_wgrad(const uint16_t* tP, const uint16_t* tS, int32_t a_tiles, const uint16_t* Aps, int32_t G, int32_t Bp,
                                   int32_t splits, float* slabP, float* slabS, void* stream) {
  if (!tP || !tS || !Aps || !slabP || !slabS) return fail(SPV_ERR_ARG, "spv_dec_heads_wgrad: null pointer%s");
  // (a workgroup walks DH_BM = 128 genes: gene tiles up to round_up(G, 128) / 32 of every cell tile are what the kernel reads)
  if (G <= 0 || Bp <= 0 || (Bp % DH_BK) != 0 || splits <= 0 || (long)a_tiles * 32 < ((long)G + DH_BM - 1) / DH_BM * DH_BM)
    return fail(SPV_ERR_ARG, "spv_dec_heads_wgrad: Bp must be a multiple of 64 and the tile arrays must cover round_up(G, 128) genes%s");
  if (!aligned16(tP, tS, Aps)) return fail(SPV_ERR_ARG, "spv_dec_heads_wgrad: operands must be 16-byte aligned%s");
  const int mtiles = (G + DH_BM - 1) / DH_BM, ktiles = Bp / DH_BK;
  const int k_per_split = (ktiles + splits - 1) / splits * DH_BK;
  launch_lds<dec_heads_wgrad_dma_kernel>(dim3(mtiles * splits), dim3(512), DH_LDS_BYTES, (hipStream_t)stream, (const bf16_t*)tP, (const bf16_t*)tS, a_tiles,
                                         (const bf16_t*)Aps, G, Bp, k_per_split, splits, slabP, slabS);
  return launch_status("spv_dec_heads_wgrad");
}

// ---------------------------------------------------------------------------------------------
// decoder / likelihood
// ---------------------------------------------------------------------------------------------
static int to_dec(const spv_dec_params* q, DecParams& p) {
  if (!q) return fail(SPV_ERR_ARG, "decoder: null params%s");
  p.X = q->X; p.ldx = q->ldx; p.rows = q->rows; p.col_off = q->col_off; p.count_is_u16 = q->count_is_u16;
  p.B = q->B; p.G = q->G; p.Bp = q->Bp; p.Gp = q->Gp;
  p.logits = q->logits; p.n_gene_tiles = q->n_gene_tiles; p.logits_f32 = q->logits_f32;
  p.Wps_hi = q->Wps_hi; p.Wps_lo = q->Wps_lo; p.Aps_hi = q->Aps_hi; p.Aps_lo = q->Aps_lo;
  p.gene_tab = (const float4*)q->gene_tab; p.cnt_tab = (const float2*)q->cnt_tab;
  p.a_p = q->a_p; p.a_s = q->a_s; p.lse_p = q->lse_p; p.lse_s = q->lse_s; p.w_row = q->w_row;
  p.gene_splits = q->gene_splits; p.genes_per_split = q->genes_per_split;
  p.part_max_p = q->part_max_p; p.part_sum_p = q->part_sum_p; p.part_max_s = q->part_max_s; p.part_sum_s = q->part_sum_s;
  p.rec_part = q->rec_part; p.tp_part = q->tp_part; p.ts_part = q->ts_part; p.dtheta_part = q->dtheta_part;
  p.dL = q->dL; p.tP = q->tP; p.tS = q->tS; p.grads_f32 = q->grads_f32;
  p.nb_splits = q->nb_splits; p.nb_genes_per_split = q->nb_genes_per_split; p.nb_cell_tiles = q->nb_cell_tiles > 0 ? q->nb_cell_tiles : 1;
  if (p.B <= 0 || p.G <= 0 || p.Bp < p.B || p.Gp < p.G || (p.Bp % DEC_CELLS_PER_WG) || (p.Gp % 32))
    return fail(SPV_ERR_ARG, "decoder: Bp must be a multiple of 128 and Gp of 32%s");
  if ((long)p.Bp * p.Gp * (p.grads_f32 ? 2 : 1) >= (1L << 30) || p.Gp >= (1 << 24))   // the likelihood kernel addresses its [Bp][Gp] arrays (two planes with grads_f32) with 32-bit byte offsets
    return fail(SPV_ERR_ARG, "decoder: Bp * Gp must stay below 2^30 elements (and Gp below 2^24)%s");
  if (p.gene_splits <= 0 || (p.genes_per_split % 32) || (long)p.gene_splits * p.genes_per_split < p.G)
    return fail(SPV_ERR_ARG, "decoder: gene splits must be multiples of 32 covering G%s");
  if (!p.Wps_hi || !p.Wps_lo || !p.Aps_hi || !p.Aps_lo) return fail(SPV_ERR_ARG, "decoder: missing packed regressor operands%s");
  if (q->kslots != 0 && q->kslots != 1) return fail(SPV_ERR_ARG, "decoder: kslots must be 0 (16 / 32 K slots) or 1 (32 / 64)%s");
  return SPV_OK;
}
// KW template argument of the kernels that read the regressor operand images: 1 = narrow layout [.][48], 2 = wide [.][96]
static inline int dec_kw(const spv_dec_params* q) { return q->kslots ? 2 : 1; }

extern "C" int spv_dec_tables(const float* px_r, int32_t G, int32_t Gp, void* gene_tab, void* cnt_tab, void* stream) {
  if (!px_r || !gene_tab || !cnt_tab || G <= 0 || Gp < G) return fail(SPV_ERR_ARG, "spv_dec_tables: bad arguments%s");
  hipLaunchKernelGGL(nb_tables_kernel, dim3((Gp + 255) / 256, NB_CMAX), dim3(256), 0, (hipStream_t)stream, px_r, G, Gp,
                     (float4*)gene_tab, (float2*)cnt_tab);
  return launch_status("spv_dec_tables");
}

// ---- the decoder's per-group launches for BOTH groups of a step in one grid each (spv_dec_group; csrc/spv_decoder.h: *_pair_kernel) ------
// Two groups whose launches take the same kernel variant go out as one grid (group = blockIdx.z); anything else falls back to the
// per-group entry points in order.
extern "C" int spv_dec_tables_grouped(const spv_dec_group* g, int32_t n, void* stream) {
  if (!g || n <= 0) return fail(SPV_ERR_ARG, "spv_dec_tables_grouped: bad arguments%s");
  return pairs_then_rest(n,
    [&](int i) {
      const spv_dec_group &a = g[i], &b = g[i + 1];
      if (!a.px_r || !b.px_r || !a.p.gene_tab || !b.p.gene_tab || !a.p.cnt_tab || !b.p.cnt_tab || a.p.G <= 0 || b.p.G <= 0 || a.p.Gp < a.p.G || b.p.Gp < b.p.G)
        return fail(SPV_ERR_ARG, "spv_dec_tables_grouped: bad arguments%s");
      const NbTabArgs a0{a.px_r, a.p.G, a.p.Gp, (float4*)a.p.gene_tab, (float2*)a.p.cnt_tab}, a1{b.px_r, b.p.G, b.p.Gp, (float4*)b.p.gene_tab, (float2*)b.p.cnt_tab};
      hipLaunchKernelGGL(nb_tables_pair_kernel, dim3((max2(a.p.Gp, b.p.Gp) + 255) / 256, NB_CMAX, 2), dim3(256), 0, (hipStream_t)stream, a0, a1);
      return launch_status("spv_dec_tables_grouped");
    },
    [&](int i) { return spv_dec_tables(g[i].px_r, g[i].p.G, g[i].p.Gp, const_cast<void*>(g[i].p.gene_tab), const_cast<void*>(g[i].p.cnt_tab), stream); });
}

static int lse_prepare(const spv_dec_params* q, const float* library, DecParams& p) {
  int rc = to_dec(q, p);
  if (rc != SPV_OK) return rc;
  if (!library || !p.part_max_p || !p.part_sum_p || !p.part_max_s || !p.part_sum_s || !p.lse_p || !p.lse_s || !p.a_p || !p.a_s)
    return fail(SPV_ERR_ARG, "spv_dec_lse: null pointer%s");
  return SPV_OK;
}
extern "C" int spv_dec_lse(const spv_dec_params* q, const float* library, void* stream) {
  DecParams p;
  int rc = lse_prepare(q, library, p);
  if (rc != SPV_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (dec_kw(q) == 2) hipLaunchKernelGGL(dec_lse_kernel<2>, dim3(p.Bp / DEC_CELLS_PER_WG, p.gene_splits), dim3(256), 0, s, p);
  else hipLaunchKernelGGL(dec_lse_kernel<1>, dim3(p.Bp / DEC_CELLS_PER_WG, p.gene_splits), dim3(256), 0, s, p);
  hipLaunchKernelGGL(dec_lse_combine_kernel, dim3((p.Bp + 63) / 64), dim3(256), 0, s, p.part_max_p, p.part_sum_p,
                     p.part_max_s, p.part_sum_s, p.gene_splits, p.Bp, p.B, library, (float*)p.lse_p, (float*)p.lse_s,
                     (float*)p.a_p, (float*)p.a_s);
  return launch_status("spv_dec_lse");
}
extern "C" int spv_dec_lse_grouped(const spv_dec_group* g, int32_t n, void* stream) {
  if (!g || n <= 0) return fail(SPV_ERR_ARG, "spv_dec_lse_grouped: bad arguments%s");
  hipStream_t s = (hipStream_t)stream;
  return pairs_then_rest(n,
    [&](int i) {
      DecParams p0, p1;
      int rc = lse_prepare(&g[i].p, g[i].library, p0);
      if (rc != SPV_OK) return rc;
      rc = lse_prepare(&g[i + 1].p, g[i + 1].library, p1);
      if (rc != SPV_OK) return rc;
      if (dec_kw(&g[i].p) != dec_kw(&g[i + 1].p)) return NOT_A_PAIR;   // (one grid needs one operand layout)
      const int bp = max2(p0.Bp, p1.Bp), gs = max2(p0.gene_splits, p1.gene_splits);
      if (dec_kw(&g[i].p) == 2) hipLaunchKernelGGL(dec_lse_pair_kernel<2>, dim3(bp / DEC_CELLS_PER_WG, gs, 2), dim3(256), 0, s, p0, p1);
      else hipLaunchKernelGGL(dec_lse_pair_kernel<1>, dim3(bp / DEC_CELLS_PER_WG, gs, 2), dim3(256), 0, s, p0, p1);
      const LseCombArgs c0{p0.part_max_p, p0.part_sum_p, p0.part_max_s, p0.part_sum_s, p0.gene_splits, p0.Bp, p0.B, g[i].library, (float*)p0.lse_p, (float*)p0.lse_s, (float*)p0.a_p, (float*)p0.a_s};
      const LseCombArgs c1{p1.part_max_p, p1.part_sum_p, p1.part_max_s, p1.part_sum_s, p1.gene_splits, p1.Bp, p1.B, g[i + 1].library, (float*)p1.lse_p, (float*)p1.lse_s, (float*)p1.a_p, (float*)p1.a_s};
      hipLaunchKernelGGL(dec_lse_combine_pair_kernel, dim3((bp + 63) / 64, 1, 2), dim3(256), 0, s, c0, c1);
      return launch_status("spv_dec_lse_grouped");
    },
    [&](int i) { return spv_dec_lse(&g[i].p, g[i].library, stream); });
}

// ---- the likelihood kernel: dec_nb_kernel for one group, dec_nb_pair_kernel for two in one grid (p1 != NULL) -----------------------------
// count storage of a group: 16-bit counts are read four at a time when base, row pitch and column offset allow 8-byte loads
static int nb_count_mode(const DecParams& p) {
  if (!p.count_is_u16) return CNT_F32;
  const bool aligned = ((reinterpret_cast<uintptr_t>(p.X) & 7) == 0) && (p.ldx % 4 == 0) && (p.col_off % 4 == 0);
  return aligned ? CNT_U16_ALIGNED : CNT_U16_ANY;
}
template <bool TRAIN, typename GT, typename LT, int CM, int KW>
static void nb_launch_as(const DecParams& p0, const DecParams* p1, hipStream_t s) {
  auto gx = [](const DecParams& p) { return ((p.Bp + NB_CELLS_PER_WG - 1) / NB_CELLS_PER_WG + p.nb_cell_tiles - 1) / p.nb_cell_tiles; };
  if (!p1) hipLaunchKernelGGL((dec_nb_kernel<TRAIN, GT, LT, CM, KW>), dim3(gx(p0), p0.nb_splits), dim3(256), 0, s, p0);
  else hipLaunchKernelGGL((dec_nb_pair_kernel<TRAIN, GT, LT, CM, KW>), dim3(max2(gx(p0), gx(*p1)), max2(p0.nb_splits, p1->nb_splits), 2), dim3(256), 0, s, p0, *p1);
}
// the kernel variant of p0 (a pair: of both groups, spv_dec_nb_fwd_grouped sees to it), resolved one template argument per step
template <bool TRAIN, typename GT, int CM, int KW>
static void nb_launch_lt(const DecParams& p0, const DecParams* p1, hipStream_t s) {
  if (p0.logits_f32) nb_launch_as<TRAIN, GT, float, CM, KW>(p0, p1, s);
  else nb_launch_as<TRAIN, GT, _Float16, CM, KW>(p0, p1, s);
}
template <bool TRAIN, typename GT, int CM>
static void nb_launch_kw(const DecParams& p0, const DecParams* p1, int kw, hipStream_t s) {
  if (kw == 2) nb_launch_lt<TRAIN, GT, CM, 2>(p0, p1, s);
  else nb_launch_lt<TRAIN, GT, CM, 1>(p0, p1, s);
}
template <bool TRAIN, typename GT>
static void nb_launch_cm(const DecParams& p0, const DecParams* p1, int kw, hipStream_t s) {
  const int cm = nb_count_mode(p0);
  if (cm == CNT_F32) nb_launch_kw<TRAIN, GT, CNT_F32>(p0, p1, kw, s);
  else if (cm == CNT_U16_ALIGNED) nb_launch_kw<TRAIN, GT, CNT_U16_ALIGNED>(p0, p1, kw, s);
  else nb_launch_kw<TRAIN, GT, CNT_U16_ANY>(p0, p1, kw, s);
}
static void nb_launch(const DecParams& p0, const DecParams* p1, int train, int kw, hipStream_t s) {
  if (!train) nb_launch_cm<false, bf16_t>(p0, p1, kw, s);
  else if (p0.grads_f32) nb_launch_cm<true, split_t>(p0, p1, kw, s);
  else nb_launch_cm<true, bf16_t>(p0, p1, kw, s);
}

static int nb_prepare(const spv_dec_params* q, int32_t train, DecParams& p) {
  int rc = to_dec(q, p);
  if (rc != SPV_OK) return rc;
  if (!p.X || !p.logits || !p.gene_tab || !p.cnt_tab || !p.a_p || !p.a_s || !p.w_row || !p.rec_part)
    return fail(SPV_ERR_ARG, "spv_dec_nb_fwd: null pointer%s");
  if (p.n_gene_tiles != p.Gp / 32) return fail(SPV_ERR_ARG, "spv_dec_nb_fwd: n_gene_tiles must be Gp / 32%s");
  if (p.nb_splits <= 0 || p.nb_genes_per_split <= 0 || (p.nb_genes_per_split % 32) || p.nb_genes_per_split > NB_GSPL_MAX ||
      (long)p.nb_splits * p.nb_genes_per_split < p.G)
    return fail(SPV_ERR_ARG, "spv_dec_nb_fwd: nb_genes_per_split must be a multiple of 32, at most 160, and the splits must cover G%s");
  if (train && (!p.dL || !p.tP || !p.tS || !p.tp_part || !p.ts_part || !p.dtheta_part))
    return fail(SPV_ERR_ARG, "spv_dec_nb_fwd: training outputs missing%s");
  return SPV_OK;
}
extern "C" int spv_dec_nb_fwd(const spv_dec_params* q, int32_t train, void* stream) {
  DecParams p;
  int rc = nb_prepare(q, train, p);
  if (rc != SPV_OK) return rc;
  nb_launch(p, nullptr, train, dec_kw(q), (hipStream_t)stream);
  return launch_status("spv_dec_nb_fwd");
}
extern "C" int spv_dec_nb_fwd_grouped(const spv_dec_group* g, int32_t n, int32_t train, void* stream) {
  if (!g || n <= 0) return fail(SPV_ERR_ARG, "spv_dec_nb_fwd_grouped: bad arguments%s");
  return pairs_then_rest(n,
    [&](int i) {
      DecParams p0, p1;
      int rc = nb_prepare(&g[i].p, train, p0);
      if (rc != SPV_OK) return rc;
      rc = nb_prepare(&g[i + 1].p, train, p1);
      if (rc != SPV_OK) return rc;
      // one grid needs one kernel variant: count storage, logits type and gradient word type of both groups must agree
      if (nb_count_mode(p0) != nb_count_mode(p1) || p0.logits_f32 != p1.logits_f32 || p0.grads_f32 != p1.grads_f32 || dec_kw(&g[i].p) != dec_kw(&g[i + 1].p)) return NOT_A_PAIR;
      nb_launch(p0, &p1, train, dec_kw(&g[i].p), (hipStream_t)stream);
      return launch_status("spv_dec_nb_fwd_grouped");
    },
    [&](int i) { return spv_dec_nb_fwd(&g[i].p, train, stream); });
}

extern "C" int spv_dec_logits(const uint16_t* Am_hi, const uint16_t* Am_lo, const uint16_t* Wm_hi, const uint16_t* Wm_lo,
                              int32_t K, int32_t Bp, int32_t Gp, int32_t nsplit, void* out, int32_t out_f32, void* stream) {
  if (!Am_hi || !Wm_hi || !out) return fail(SPV_ERR_ARG, "spv_dec_logits: null pointer%s");
  if (K <= 0 || (K % 32) || Bp <= 0 || Gp <= 0 || (Bp % 128) || (Gp % 128)) return fail(SPV_ERR_ARG, "spv_dec_logits: bad shape%s");
  if (nsplit != 1 && nsplit != 3) return fail(SPV_ERR_ARG, "spv_dec_logits: nsplit must be 1 or 3%s");
  if (nsplit == 3 && (!Am_lo || !Wm_lo)) return fail(SPV_ERR_ARG, "spv_dec_logits: nsplit=3 needs lo images%s");
  // genes on MFMA rows (M), cells on MFMA columns (N): the orientation the likelihood kernel consumes
  GemmParams p{};
  p.A = Wm_hi; p.A_lo = Wm_lo; p.lda = K;
  p.B = Am_hi; p.B_lo = Am_lo; p.ldb = K;
  p.C = (float*)out; p.ldc = 0; p.slab_stride = 0;
  p.M = Gp; p.N = Bp; p.K = K; p.k_per_split = K;
  p.epi = out_f32 ? EPI_TILED_F32 : EPI_TILED_F16;
  p.tiles_inner = Gp / 32;
  hipStream_t s = (hipStream_t)stream;
  if (nsplit == 1 && !out_f32 && Gp % DL_BM == 0 && Bp % DL_BN == 0 && aligned16(Am_hi, Wm_hi)) {
    // LDS-DMA kernel (spv_dec_gemm.h): 256 x 128 tiles, two workgroups per CU
    launch_lds<dec_logits_dma_kernel>(dim3(Gp / DL_BM, Bp / DL_BN), dim3(512), DL_LDS_BYTES, s, (const bf16_t*)Wm_hi, (const bf16_t*)Am_hi, K, Gp / 32, (_Float16*)out);
    return launch_status("spv_dec_logits dma");
  }
  if (nsplit == 3) launch_gemm<GemmCfg<128, 128, 2, 2, false, false, SRC_PLAIN, SRC_PLAIN, unsigned short, 3, 32, 4>>(p, 1, s);
  else if (Gp % 256 == 0) launch_gemm<GemmCfg<256, 128, 2, 2, false, false, SRC_PLAIN, SRC_PLAIN, unsigned short, 1, 32, 2, 2>>(p, 1, s);  // 128 x 64 wave tiles: 25 % less LDS traffic per MFMA
  else launch_gemm<GemmCfg<128, 128, 2, 2, false, false, SRC_PLAIN, SRC_PLAIN, unsigned short, 1, 32, 4>>(p, 1, s);
  return launch_status("spv_dec_logits");
}

static bool logits_dma_ok(const spv_dec_group& a) {
  return a.Am_hi && a.Wm_hi && a.p.logits && a.nsplit == 1 && !a.p.logits_f32 && a.K > 0 && (a.K % 32) == 0 && a.p.Bp > 0 && a.p.Gp > 0 &&
         a.p.Gp % DL_BM == 0 && a.p.Bp % DL_BN == 0 && aligned16(a.Am_hi, a.Wm_hi);
}
extern "C" int spv_dec_logits_grouped(const spv_dec_group* g, int32_t n, void* stream) {
  if (!g || n <= 0) return fail(SPV_ERR_ARG, "spv_dec_logits_grouped: bad arguments%s");
  return pairs_then_rest(n,
    [&](int i) {
      const spv_dec_group &a = g[i], &b = g[i + 1];
      if (!(logits_dma_ok(a) && logits_dma_ok(b))) return NOT_A_PAIR;
      const LogitsArgs a0{(const bf16_t*)a.Wm_hi, (const bf16_t*)a.Am_hi, a.K, a.p.Gp / 32, a.p.Bp, (_Float16*)const_cast<void*>(a.p.logits)};
      const LogitsArgs a1{(const bf16_t*)b.Wm_hi, (const bf16_t*)b.Am_hi, b.K, b.p.Gp / 32, b.p.Bp, (_Float16*)const_cast<void*>(b.p.logits)};
      launch_lds<dec_logits_dma_pair_kernel>(dim3(max2(a.p.Gp, b.p.Gp) / DL_BM, max2(a.p.Bp, b.p.Bp) / DL_BN, 2), dim3(512), DL_LDS_BYTES, (hipStream_t)stream, a0, a1);
      return launch_status("spv_dec_logits_grouped");
    },
    [&](int i) {
      const spv_dec_group& a = g[i];
      return spv_dec_logits(a.Am_hi, a.Am_lo, a.Wm_hi, a.Wm_lo, a.K, a.p.Bp, a.p.Gp, a.nsplit, const_cast<void*>(a.p.logits), a.p.logits_f32, stream);
    });
}

extern "C" int spv_dec_materialize(const spv_dec_params* q, float* scale_p, float* scale_s, float* rate_p, float* rate_s,
                                   float* logits_out, int64_t ld, void* stream) {
  DecParams p;
  int rc = to_dec(q, p);
  if (rc != SPV_OK) return rc;
  if (!scale_p || !scale_s || !rate_p || !rate_s || !logits_out || ld < p.G || !p.logits || !p.lse_p || !p.lse_s || !p.a_p || !p.a_s)
    return fail(SPV_ERR_ARG, "spv_dec_materialize: null pointer / ld < G%s");
  if (p.n_gene_tiles != p.Gp / 32) return fail(SPV_ERR_ARG, "spv_dec_materialize: n_gene_tiles must be Gp / 32%s");
  dim3 grid(p.Bp / DEC_CELLS_PER_WG, p.gene_splits);
  hipStream_t s = (hipStream_t)stream;
  const bool wide = dec_kw(q) == 2;
  if (p.logits_f32 && wide) hipLaunchKernelGGL((dec_materialize_kernel<float, 2>), grid, dim3(256), 0, s, p, scale_p, scale_s, rate_p, rate_s, logits_out, (long)ld);
  else if (p.logits_f32) hipLaunchKernelGGL((dec_materialize_kernel<float>), grid, dim3(256), 0, s, p, scale_p, scale_s, rate_p, rate_s, logits_out, (long)ld);
  else if (wide) hipLaunchKernelGGL((dec_materialize_kernel<_Float16, 2>), grid, dim3(256), 0, s, p, scale_p, scale_s, rate_p, rate_s, logits_out, (long)ld);
  else hipLaunchKernelGGL((dec_materialize_kernel<_Float16>), grid, dim3(256), 0, s, p, scale_p, scale_s, rate_p, rate_s, logits_out, (long)ld);
  return launch_status("spv_dec_materialize");
}

// What spv_dec_expected and spv_dec_sample share ahead of their launches: the decoder parameters, the checks of the logits operands and
// of the gene selection (reported under the entry point's name ``who``), and the grid.  X: either argument struct.
template <typename X>
static int readout_prepare(const spv_dec_params* q, const char* who, const X* x, DecParams& p, dim3& grid) {
  int rc = to_dec(q, p);
  if (rc != SPV_OK) return rc;
  if (!x) return fail(SPV_ERR_ARG, "%s: null arguments", who);
  if (!p.a_p || !p.a_s || !x->Am_hi || !x->Wm_hi || !x->out) return fail(SPV_ERR_ARG, "%s: null pointer", who);
  if (x->K <= 0 || (x->K % 32) || x->K > DX_KMAX) return fail(SPV_ERR_ARG, "%s: K must be a multiple of 32, at most 320", who);
  if (x->nsplit != 1 && x->nsplit != 3) return fail(SPV_ERR_ARG, "%s: nsplit must be 1 or 3", who);
  if (x->nsplit == 3 && (!x->Am_lo || !x->Wm_lo)) return fail(SPV_ERR_ARG, "%s: nsplit=3 needs lo images", who);
  if (!aligned16(x->Am_hi, x->Wm_hi, x->Am_lo, x->Wm_lo))
    return fail(SPV_ERR_ARG, "%s: operand images must be 16-byte aligned", who);
  if (x->n_genes <= 0 || (!x->genes && x->n_genes > p.G)) return fail(SPV_ERR_ARG, "%s: n_genes must be positive (and at most G without a gene list)", who);
  // one workgroup per 32 cells and gene slice; each of its 4 waves walks every (4 gy)-th 32-gene tile.  ~8 workgroups per CU keep
  // the gathers of the gene rows covered; never more slices than there are tiles for the waves.
  const int gx = p.Bp / DX_CELLS, tiles = (x->n_genes + 31) / 32;
  int gy = (2048 + gx - 1) / gx;
  if (gy > (tiles + 3) / 4) gy = (tiles + 3) / 4;
  if (gy < 1) gy = 1;
  grid = dim3(gx, gy);
  return SPV_OK;
}

extern "C" int spv_dec_expected(const spv_dec_params* q, const spv_dec_expected_args* x, void* stream) {
  DecParams p;
  dim3 grid;
  int rc = readout_prepare(q, "spv_dec_expected", x, p, grid);
  if (rc != SPV_OK) return rc;
  if (x->what < 0 || x->what > 3) return fail(SPV_ERR_ARG, "spv_dec_expected: what must be 0 (mixture), 1 (private), 2 (shared) or 3 (mixing weight)%s");
  if (x->ld_out < x->n_genes) return fail(SPV_ERR_ARG, "spv_dec_expected: ld_out < n_genes%s");
  const DecExpArgs a{(const bf16_t*)x->Am_hi, (const bf16_t*)x->Am_lo, (const bf16_t*)x->Wm_hi, (const bf16_t*)x->Wm_lo, x->K,
                     x->genes, x->n_genes, x->what, x->out, (long)x->ld_out, x->alpha, x->accumulate};
  hipStream_t s = (hipStream_t)stream;
  const bool wide = dec_kw(q) == 2;
  if (x->nsplit == 3 && wide) hipLaunchKernelGGL((dec_expected_kernel<3, 2>), grid, dim3(256), 0, s, p, a);
  else if (x->nsplit == 3) hipLaunchKernelGGL((dec_expected_kernel<3, 1>), grid, dim3(256), 0, s, p, a);
  else if (wide) hipLaunchKernelGGL((dec_expected_kernel<1, 2>), grid, dim3(256), 0, s, p, a);
  else hipLaunchKernelGGL((dec_expected_kernel<1, 1>), grid, dim3(256), 0, s, p, a);
  return launch_status("spv_dec_expected");
}

extern "C" int spv_dec_sample(const spv_dec_params* q, const spv_dec_sample_args* x, void* stream) {
  DecParams p;
  dim3 grid;
  int rc = readout_prepare(q, "spv_dec_sample", x, p, grid);
  if (rc != SPV_OK) return rc;
  if (!x->theta) return fail(SPV_ERR_ARG, "spv_dec_sample: null pointer%s");
  if (x->ld_gene < 1) return fail(SPV_ERR_ARG, "spv_dec_sample: ld_gene < 1%s");
  if (x->ld_out < (int64_t)(x->n_genes - 1) * x->ld_gene + 1) return fail(SPV_ERR_ARG, "spv_dec_sample: ld_out < (n_genes - 1) * ld_gene + 1%s");
  const DecSampleArgs a{(const bf16_t*)x->Am_hi, (const bf16_t*)x->Am_lo, (const bf16_t*)x->Wm_hi, (const bf16_t*)x->Wm_lo, x->K,
                        x->genes, x->n_genes, x->theta, x->cell_ids, (unsigned long long)x->key, x->sample, x->out, (long)x->ld_out, x->ld_gene};
  hipStream_t s = (hipStream_t)stream;
  const bool wide = dec_kw(q) == 2;
  if (x->nsplit == 3 && wide) hipLaunchKernelGGL((dec_sample_kernel<3, 2>), grid, dim3(256), 0, s, p, a);
  else if (x->nsplit == 3) hipLaunchKernelGGL((dec_sample_kernel<3, 1>), grid, dim3(256), 0, s, p, a);
  else if (wide) hipLaunchKernelGGL((dec_sample_kernel<1, 2>), grid, dim3(256), 0, s, p, a);
  else hipLaunchKernelGGL((dec_sample_kernel<1, 1>), grid, dim3(256), 0, s, p, a);
  return launch_status("spv_dec_sample");
}

extern "C" int spv_dec_sample_stats(const spv_dec_params* q, const spv_dec_sample_stats_args* x, void* stream) {
  DecParams p;
  dim3 grid;
  // readout_prepare checks the fields the read-outs share under spv_dec_sample's names: the table stands in for its `out`
  spv_dec_sample_args y{};
  if (x) {
    y.Am_hi = x->Am_hi; y.Am_lo = x->Am_lo; y.Wm_hi = x->Wm_hi; y.Wm_lo = x->Wm_lo; y.K = x->K; y.nsplit = x->nsplit;
    y.genes = x->genes; y.n_genes = x->n_genes; y.out = reinterpret_cast<int32_t*>(x->stats);
  }
  int rc = readout_prepare(q, "spv_dec_sample_stats", x ? &y : nullptr, p, grid);
  if (rc != SPV_OK) return rc;
  if (!x->theta) return fail(SPV_ERR_ARG, "spv_dec_sample_stats: null pointer%s");
  if (x->n_seg < 1) return fail(SPV_ERR_ARG, "spv_dec_sample_stats: n_seg < 1%s");
  if (x->ld_stats < x->n_genes) return fail(SPV_ERR_ARG, "spv_dec_sample_stats: ld_stats < n_genes%s");
  const DecSampleStatsArgs a{(const bf16_t*)x->Am_hi, (const bf16_t*)x->Am_lo, (const bf16_t*)x->Wm_hi, (const bf16_t*)x->Wm_lo, x->K,
                             x->genes, x->n_genes, x->theta, x->cell_ids, (unsigned long long)x->key, x->sample, x->seg, x->n_seg,
                             (unsigned long long*)x->stats, (long)x->ld_stats, (unsigned long long*)x->cell_total};
  hipStream_t s = (hipStream_t)stream;
  const bool wide = dec_kw(q) == 2;
  if (x->nsplit == 3 && wide) hipLaunchKernelGGL((dec_sample_stats_kernel<3, 2>), grid, dim3(256), 0, s, p, a);
  else if (x->nsplit == 3) hipLaunchKernelGGL((dec_sample_stats_kernel<3, 1>), grid, dim3(256), 0, s, p, a);
  else if (wide) hipLaunchKernelGGL((dec_sample_stats_kernel<1, 2>), grid, dim3(256), 0, s, p, a);
  else hipLaunchKernelGGL((dec_sample_stats_kernel<1, 1>), grid, dim3(256), 0, s, p, a);
  return launch_status("spv_dec_sample_stats");
}

extern "C" int64_t spv_dec_expected_stats_ws_bytes(int32_t n_genes, int32_t n_cell_tiles) {
  if (n_genes <= 0 || n_cell_tiles <= 0) return 0;
  return (int64_t)n_cell_tiles * DXS_ROWS * n_genes * (int64_t)sizeof(double);
}

extern "C" int spv_dec_expected_stats(const spv_dec_params* q, const spv_dec_expected_stats_args* x, void* stream) {
  DecParams p;
  dim3 grid;
  // readout_prepare checks the fields the read-outs share under spv_dec_expected's names: the table stands in for its `out`
  spv_dec_expected_args y{};
  if (x) {
    y.Am_hi = x->Am_hi; y.Am_lo = x->Am_lo; y.Wm_hi = x->Wm_hi; y.Wm_lo = x->Wm_lo; y.K = x->K; y.nsplit = x->nsplit;
    y.genes = x->genes; y.n_genes = x->n_genes; y.out = reinterpret_cast<float*>(x->stats);
  }
  int rc = readout_prepare(q, "spv_dec_expected_stats", x ? &y : nullptr, p, grid);
  if (rc != SPV_OK) return rc;
  if (!x->ws) return fail(SPV_ERR_ARG, "spv_dec_expected_stats: null workspace%s");
  if (!x->tile_seg) return fail(SPV_ERR_ARG, "spv_dec_expected_stats: null tile_seg%s");
  if (!x->tile_n) return fail(SPV_ERR_ARG, "spv_dec_expected_stats: null tile_n%s");
  if (x->n_seg < 1) return fail(SPV_ERR_ARG, "spv_dec_expected_stats: n_seg < 1%s");
  if (x->ld_stats < x->n_genes) return fail(SPV_ERR_ARG, "spv_dec_expected_stats: ld_stats < n_genes%s");
  const DecExpStatsArgs a{(const bf16_t*)x->Am_hi, (const bf16_t*)x->Am_lo, (const bf16_t*)x->Wm_hi, (const bf16_t*)x->Wm_lo, x->K,
                          x->genes, x->n_genes, x->n_seg, x->tile_seg, x->tile_n, x->ws};
  hipStream_t s = (hipStream_t)stream;
  const bool wide = dec_kw(q) == 2;
  if (x->nsplit == 3 && wide) hipLaunchKernelGGL((dec_expected_stats_kernel<3, 2>), grid, dim3(256), 0, s, p, a);
  else if (x->nsplit == 3) hipLaunchKernelGGL((dec_expected_stats_kernel<3, 1>), grid, dim3(256), 0, s, p, a);
  else if (wide) hipLaunchKernelGGL((dec_expected_stats_kernel<1, 2>), grid, dim3(256), 0, s, p, a);
  else hipLaunchKernelGGL((dec_expected_stats_kernel<1, 1>), grid, dim3(256), 0, s, p, a);
  rc = launch_status("spv_dec_expected_stats");
  if (rc != SPV_OK) return rc;
  // the tiles' partial sums -> the table: one thread per (row, gene), the cell tiles in ascending order
  hipLaunchKernelGGL(dec_expected_stats_merge_kernel, dim3((x->n_genes + 255) / 256, DXS_ROWS), dim3(256), 0, s, x->tile_seg, x->tile_n,
                     p.Bp / DX_CELLS, x->n_seg, p.B, x->n_genes, (const double*)x->ws, x->stats, (long)x->ld_stats);
  return launch_status("spv_dec_expected_stats");
}

extern "C" int spv_nbmix_sample(const float* rate_p, const float* rate_s, const float* logit, int64_t ld_in, const float* theta, int32_t R, int32_t G,
                                const int32_t* cell_ids, uint64_t key, uint32_t sample, int32_t* out, int64_t ld_out, void* stream) {
  if (!rate_p || !rate_s || !logit || !theta || !out) return fail(SPV_ERR_ARG, "spv_nbmix_sample: null pointer%s");
  if (R < 0 || G <= 0) return fail(SPV_ERR_ARG, "spv_nbmix_sample: R must not be negative, G must be positive%s");
  if (ld_in < G || ld_out < G) return fail(SPV_ERR_ARG, "spv_nbmix_sample: ld_in and ld_out must be at least G%s");
  if (R == 0) return SPV_OK;
  const long n = (long)R * G;
  if ((n + 255) / 256 > 0x7fffffffL) return fail(SPV_ERR_ARG, "spv_nbmix_sample: R * G exceeds the grid%s");
  const NbMixArgs a{rate_p, rate_s, logit, (long)ld_in, theta, R, G, cell_ids, (unsigned long long)key, sample, out, (long)ld_out};
  hipLaunchKernelGGL(nbmix_sample_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  return launch_status("spv_nbmix_sample");
}

extern "C" int32_t spv_de_pairs_splits(int32_t n_genes, int32_t n_pairs) {
  if (n_genes <= 0 || n_pairs <= 0) return 0;
  return de_splits(n_genes, n_pairs);
}

extern "C" int spv_de_pairs(const spv_de_pairs_args* x, void* stream) {
  if (!x) return fail(SPV_ERR_ARG, "spv_de_pairs: null arguments%s");
  if (!x->bank1 || !x->bank2 || !x->rows1 || !x->rows2 || !x->stats || !x->ws) return fail(SPV_ERR_ARG, "spv_de_pairs: null pointer%s");
  if (x->n_pairs <= 0 || x->n_pairs > (1 << 24)) return fail(SPV_ERR_ARG, "spv_de_pairs: n_pairs must lie in [1, 2^24]%s");
  if (x->n_genes <= 0 || x->n_rows1 <= 0 || x->n_rows2 <= 0) return fail(SPV_ERR_ARG, "spv_de_pairs: n_genes and the banks' row counts must be positive%s");
  if (x->ld1 < x->n_genes || x->ld2 < x->n_genes || x->ld_stats < x->n_genes) return fail(SPV_ERR_ARG, "spv_de_pairs: ld < n_genes%s");
  if (!(x->delta >= 0.f) || !(x->eps >= 0.f)) return fail(SPV_ERR_ARG, "spv_de_pairs: delta and eps must be non-negative numbers%s");
  const int splits = de_splits(x->n_genes, x->n_pairs), tiles = (x->n_genes + 63) / 64;
  if (x->ws_bytes < (int64_t)splits * DE_FIELDS * x->n_genes * (int64_t)sizeof(double) || (reinterpret_cast<uintptr_t>(x->ws) & 7))
    return fail(SPV_ERR_ARG, "spv_de_pairs: the workspace must be 8-byte aligned and hold spv_de_pairs_splits() * 7 * n_genes doubles%s");
  const DeArgs a{x->bank1, x->bank2, (long)x->ld1, (long)x->ld2, x->rows1, x->rows2, x->n_rows1, x->n_rows2, x->n_genes, x->n_pairs,
                 x->delta, x->eps, x->stats, (long)x->ld_stats, (double*)x->ws, splits};
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(de_pairs_kernel, dim3((tiles * splits + 7) & ~7), dim3(64 * DE_WAVES), 0, s, a);
  int rc = launch_status("spv_de_pairs");
  if (rc != SPV_OK) return rc;
  hipLaunchKernelGGL(de_finish_kernel, dim3(tiles), dim3(64 * DE_FIN_WAVES), 0, s, a);
  return launch_status("spv_de_pairs (final combine)");
}

extern "C" int64_t spv_de_median_ws_bytes(int32_t n_genes, int32_t n_pairs) {
  if (n_genes <= 0 || n_pairs <= 0) return 0;
  return dm_ws_words(n_genes) * (int64_t)sizeof(unsigned);
}

template <int PASS>
static int de_median_pass(const DmArgs& a, int tiles, hipStream_t s) {
  hipLaunchKernelGGL((de_median_pass_kernel<PASS>), dim3((tiles * a.splits + 7) & ~7), dim3(64 * DM_WAVES), 0, s, a);
  int rc = launch_status("spv_de_median (gather pass)");
  if (rc != SPV_OK) return rc;
  hipLaunchKernelGGL(de_median_pick_kernel, dim3(tiles), dim3(256), 0, s, a, PASS);
  return launch_status("spv_de_median (bin pick)");
}

extern "C" int spv_de_median(const spv_de_median_args* x, void* stream) {
  if (!x) return fail(SPV_ERR_ARG, "spv_de_median: null arguments%s");
  if (!x->bank1 || !x->bank2 || !x->rows1 || !x->rows2 || !x->mid || !x->ws) return fail(SPV_ERR_ARG, "spv_de_median: null pointer%s");
  if (x->n_pairs <= 0 || x->n_pairs > (1 << 24)) return fail(SPV_ERR_ARG, "spv_de_median: n_pairs must lie in [1, 2^24]%s");
  if (x->n_genes <= 0 || x->n_rows1 <= 0 || x->n_rows2 <= 0) return fail(SPV_ERR_ARG, "spv_de_median: n_genes and the banks' row counts must be positive%s");
  if (x->ld1 < x->n_genes || x->ld2 < x->n_genes || x->ld_mid < x->n_genes) return fail(SPV_ERR_ARG, "spv_de_median: ld < n_genes%s");
  if (!(x->eps >= 0.f)) return fail(SPV_ERR_ARG, "spv_de_median: eps must be a non-negative number%s");
  if (x->ws_bytes < dm_ws_words(x->n_genes) * (int64_t)sizeof(unsigned) || (reinterpret_cast<uintptr_t>(x->ws) & 3))
    return fail(SPV_ERR_ARG, "spv_de_median: the workspace must be 4-byte aligned and hold spv_de_median_ws_bytes() bytes%s");
  const int tiles = (x->n_genes + 63) / 64;
  const DmArgs a{x->bank1, x->bank2, (long)x->ld1, (long)x->ld2, x->rows1, x->rows2, x->n_rows1, x->n_rows2, x->n_genes, x->n_pairs,
                 x->eps, x->mid, (long)x->ld_mid, (unsigned*)x->ws, dm_splits(x->n_genes, x->n_pairs)};
  hipStream_t s = (hipStream_t)stream;
  const long words = (long)DM_BINS * x->n_genes;
  hipLaunchKernelGGL(de_median_zero_kernel, dim3((unsigned)((words + 1023) / 1024 < 2048 ? (words + 1023) / 1024 : 2048)), dim3(256), 0, s, a.ws, words);
  int rc = launch_status("spv_de_median (clear)");
  if (rc == SPV_OK) rc = de_median_pass<0>(a, tiles, s);
  if (rc == SPV_OK) rc = de_median_pass<1>(a, tiles, s);
  if (rc == SPV_OK) rc = de_median_pass<2>(a, tiles, s);
  if (rc == SPV_OK) rc = de_median_pass<3>(a, tiles, s);
  return rc;
}

// ---------------------------------------------------------------------------------------------
// statistics of the observed counts (spv_count_stats.h)
// ---------------------------------------------------------------------------------------------
extern "C" int32_t spv_count_stats_tile(void) { return CS_TILE; }
extern "C" int32_t spv_count_stats_slab(void) { return CS_SLAB; }
extern "C" int64_t spv_count_stats_ws_bytes(int32_t G, int32_t n_slabs) {
  if (G <= 0 || n_slabs <= 0) return 0;
  return (int64_t)n_slabs * 3 * G * (int64_t)sizeof(double);
}

static int count_stats_check(const spv_count_stats_args* x, const char* who, bool partial, bool merge, CsArgs& a) {
  if (!x) return fail(SPV_ERR_ARG, "%s: null arguments", who);
  if (!x->slabs || !x->seg_slabs || !x->ws) return fail(SPV_ERR_ARG, "%s: null pointer (slabs, seg_slabs, ws)", who);
  if (x->G <= 0 || x->n_slabs <= 0 || x->n_seg <= 0) return fail(SPV_ERR_ARG, "%s: G, n_slabs and n_seg must be positive", who);
  if (x->ws_bytes < spv_count_stats_ws_bytes(x->G, x->n_slabs) || (reinterpret_cast<uintptr_t>(x->ws) & 7))
    return fail(SPV_ERR_ARG, "%s: the workspace must be 8-byte aligned and hold spv_count_stats_ws_bytes() bytes", who);
  if (partial) {
    if (!x->x.X) return fail(SPV_ERR_ARG, "%s: null count matrix", who);
    if (x->x.dtype != SPV_COUNT_U16 && x->x.dtype != SPV_COUNT_F32) return fail(SPV_ERR_ARG, "%s: unknown count dtype", who);
    if (x->n_rows <= 0 || x->n <= 0 || x->pos_off < 0 || (int64_t)x->pos_off + x->n > INT32_MAX) return fail(SPV_ERR_ARG, "%s: n_rows and n must be positive, pos_off non-negative", who);
    if (x->x.col_off < 0 || x->x.ld < (int64_t)x->x.col_off + x->G) return fail(SPV_ERR_ARG, "%s: ld < col_off + G", who);
    if (!x->x.rows && x->n > x->n_rows) return fail(SPV_ERR_ARG, "%s: without a row list n must not exceed n_rows", who);
    if (x->slab_first < 0 || x->slab_count <= 0 || (int64_t)x->slab_first + x->slab_count > x->n_slabs) return fail(SPV_ERR_ARG, "%s: slab range outside the table", who);
    if ((int64_t)x->slab_count * ((x->G + CS_TILE - 1) / CS_TILE) > INT32_MAX) return fail(SPV_ERR_ARG, "%s: too many (slab, gene tile) workgroups for one launch", who);
  }
  if (merge) {
    if (!x->out) return fail(SPV_ERR_ARG, "%s: null output", who);
    if (x->n_sel <= 0 || (!x->genes && x->n_sel > x->G)) return fail(SPV_ERR_ARG, "%s: n_sel must be positive (and at most G without a gene list)", who);
    if (x->ld_out < x->n_sel || x->n_seg > 65535) return fail(SPV_ERR_ARG, "%s: ld_out < n_sel, or more than 65535 segments", who);
  }
  a = CsArgs{x->x.X, (long)x->x.ld, x->x.rows, x->x.col_off, x->G, x->n_rows, x->n, x->pos_off, x->w, x->genes, x->n_sel, x->slabs, x->seg_slabs,
             x->n_slabs, x->n_seg, x->slab_first, x->slab_count, x->out, (long)x->ld_out, (double*)x->ws};
  return SPV_OK;
}

static int count_stats_partial_launch(const spv_count_stats_args* x, const CsArgs& a, hipStream_t s) {
  const bool u16 = x->x.dtype == SPV_COUNT_U16;
  const int64_t es = u16 ? 2 : 4;
  // 16-byte loads need every row's first gene on a 16-byte boundary (and a row that holds one whole piece: cs_load)
  const bool vec = ((reinterpret_cast<uintptr_t>(x->x.X) + (uintptr_t)(x->x.col_off * es)) & 15) == 0 && ((x->x.ld * es) & 15) == 0 && x->G * es >= 16;
  const dim3 grid((unsigned)(x->slab_count * ((x->G + CS_TILE - 1) / CS_TILE))), block(64 * CS_WAVES);
  if (u16 && vec) hipLaunchKernelGGL((count_stats_partial_kernel<true, true>), grid, block, 0, s, a);
  else if (u16) hipLaunchKernelGGL((count_stats_partial_kernel<true, false>), grid, block, 0, s, a);
  else if (vec) hipLaunchKernelGGL((count_stats_partial_kernel<false, true>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((count_stats_partial_kernel<false, false>), grid, block, 0, s, a);
  return launch_status("spv_count_stats (partial pass)");
}

static int count_stats_merge_launch(const CsArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(count_stats_merge_kernel, dim3((unsigned)((a.n_sel + 255) / 256), (unsigned)a.n_seg), dim3(256), 0, s, a);
  return launch_status("spv_count_stats (merge pass)");
}

extern "C" int spv_count_stats_partial(const spv_count_stats_args* x, void* stream) {
  CsArgs a;
  int rc = count_stats_check(x, "spv_count_stats_partial", true, false, a);
  if (rc != SPV_OK) return rc;
  return count_stats_partial_launch(x, a, (hipStream_t)stream);
}

extern "C" int spv_count_stats_merge(const spv_count_stats_args* x, void* stream) {
  CsArgs a;
  int rc = count_stats_check(x, "spv_count_stats_merge", false, true, a);
  if (rc != SPV_OK) return rc;
  return count_stats_merge_launch(a, (hipStream_t)stream);
}

extern "C" int spv_count_stats(const spv_count_stats_args* x, void* stream) {
  CsArgs a;
  int rc = count_stats_check(x, "spv_count_stats", true, true, a);
  if (rc != SPV_OK) return rc;
  if (x->slab_first != 0 || x->slab_count != x->n_slabs || x->pos_off != 0) return fail(SPV_ERR_ARG, "spv_count_stats: the whole list in one call (slab_first = pos_off = 0, slab_count = n_slabs)%s");
  rc = count_stats_partial_launch(x, a, (hipStream_t)stream);
  if (rc != SPV_OK) return rc;
  return count_stats_merge_launch(a, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------
// exact k-nearest neighbours (spv_knn.h)
// ---------------------------------------------------------------------------------------------
extern "C" int32_t spv_knn_tile_q(void) { return KNN_TQ; }
extern "C" int32_t spv_knn_tile_c(void) { return KNN_TC; }
extern "C" int32_t spv_knn_splits(int32_t n_q, int32_t n_c) { return knn_splits(n_q, n_c); }
extern "C" int64_t spv_knn_ws_bytes(int32_t n_q, int32_t k, int32_t n_split) {
  if (n_q < 1 || k < 1 || n_split <= 1) return 0;
  return (int64_t)n_split * n_q * k * 8;
}

// ---- what the entry points of the pair scan share (spv_pair_scan.h): spv_knn here, spv_ot_softmin / spv_ot_topk, spv_ot_segment_lse, spv_ot_project, spv_silhouette_sums and spv_tsne_repulsion below
struct ScanPlan { int n_split, per; dim3 grid; };   // chunks (resolved), candidates per chunk, (query tiles, chunks)

// What every one of them refuses about the two sides, D, n_split and ws, in `who`'s name; the chunks -- n_split, or splits(n_q, n_c) for
// 0 -- and the grid.  X: any of the argument structs (they share these fields).  own(n_split) checks the caller's other fields, ahead of ws.
template <typename X, typename Splits, typename Own>
static int scan_check(const X* x, const char* who, Splits splits, ScanPlan& p, Own own) {
  if (!x) return fail(SPV_ERR_ARG, "%s: null arguments", who);
  if (!x->Q) return fail(SPV_ERR_ARG, "%s: null Q", who);
  if (!x->C) return fail(SPV_ERR_ARG, "%s: null C", who);
  if (x->D < 1 || x->D > KNN_DMAX) return fail(SPV_ERR_ARG, "%s: D must lie in [1, 64]", who);
  if (x->n_split < 0 || x->n_split > KNN_SPLIT_MAX) return fail(SPV_ERR_ARG, "%s: n_split must be 0 or lie in [1, 64]", who);
  if (x->n_q < 1) return fail(SPV_ERR_ARG, "%s: n_q < 1", who);
  if (x->n_c < 0) return fail(SPV_ERR_ARG, "%s: n_c < 0", who);
  if (x->ld_q < x->D) return fail(SPV_ERR_ARG, "%s: ld_q < D", who);
  if (x->ld_c < x->D) return fail(SPV_ERR_ARG, "%s: ld_c < D", who);
  p.n_split = x->n_split ? x->n_split : splits(x->n_q, x->n_c);
  const int rc = own(p.n_split);
  if (rc != SPV_OK) return rc;
  if (p.n_split > 1 && !x->ws) return fail(SPV_ERR_ARG, "%s: null ws", who);
  if (reinterpret_cast<uintptr_t>(x->ws) & 7) return fail(SPV_ERR_ARG, "%s: ws must be 8-byte aligned", who);
  p.per = knn_chunk(x->n_c, p.n_split);
  p.grid = dim3((unsigned)((x->n_q + KNN_TQ - 1) / KNN_TQ), (unsigned)p.n_split);
  return SPV_OK;
}

// the scan kernels' form for D columns: launch(DP) with DP = 16 / 32 / 64 as a compile-time constant
template <typename Launch>
static void scan_dispatch(int D, Launch launch) {
  if (D <= 16) launch(std::integral_constant<int, 16>());
  else if (D <= 32) launch(std::integral_constant<int, 32>());
  else launch(std::integral_constant<int, 64>());
}

// (idx, values) rows of k entries, ld_out apart and indexed in 32 bits (spv_knn, spv_ot_topk)
template <typename X>
static int scan_check_rows(const X* x, const char* who) {
  if (x->k < 1 || x->k > KNN_KMAX) return fail(SPV_ERR_ARG, "%s: k must lie in [1, 64]", who);
  if (x->ld_out < x->k) return fail(SPV_ERR_ARG, "%s: ld_out < k", who);
  if ((int64_t)x->n_q * x->ld_out > INT32_MAX || x->ld_out > INT32_MAX) return fail(SPV_ERR_ARG, "%s: n_q * ld_out exceeds 2^31 - 1", who);
  return SPV_OK;
}

extern "C" int spv_knn(const spv_knn_args* x, void* stream) {
  ScanPlan p;
  int rc = scan_check(x, "spv_knn", knn_splits, p, [&](int n_split) {
    if (!x->idx) return fail(SPV_ERR_ARG, "spv_knn: null idx%s");
    if (!x->dist) return fail(SPV_ERR_ARG, "spv_knn: null dist%s");
    const int rc = scan_check_rows(x, "spv_knn");
    if (rc != SPV_OK) return rc;
    if ((int64_t)n_split * x->n_q * x->k > INT32_MAX) return fail(SPV_ERR_ARG, "spv_knn: the workspace (n_split * n_q * k entries) exceeds 2^31 - 1%s");
    return SPV_OK;
  });
  if (rc != SPV_OK) return rc;
  const KnnArgs a{x->Q, (long)x->ld_q, x->n_q, x->C, (long)x->ld_c, x->n_c, x->D, x->k, x->exclude, p.n_split, p.per,
                  x->idx, x->dist, (int)x->ld_out, (knn_key_t*)x->ws};
  hipStream_t s = (hipStream_t)stream;
  // the opt-in is to the largest LDS a call can ask for (k = SPV_KNN_KMAX: beyond the 64 KiB a kernel gets unasked), the launch takes what k needs
  scan_dispatch(a.D, [&](auto dp) { constexpr int DP = decltype(dp)::value; launch_lds_upto<knn_partial_kernel<DP>>(p.grid, dim3(KNN_TQ), knn_lds_bytes(DP, KNN_KMAX), knn_lds_bytes(DP, a.k), s, a); });
  rc = launch_status(p.n_split == 1 ? "spv_knn" : "spv_knn (partial pass)");
  if (rc != SPV_OK || p.n_split == 1) return rc;
  hipLaunchKernelGGL(knn_merge_kernel, dim3(p.grid.x), dim3(KNN_TQ), knn_lds_bytes(0, x->k), s, a);   // at most the 64 KiB a kernel gets unasked
  return launch_status("spv_knn (merge pass)");
}

// the same search for up to SPV_KNN_PAGED_KMAX neighbours: page 0 is spv_knn's two kernels as they are, every later page one more run
// of them on the candidates after the previous page's last key, which the partial pass reads from the column the previous page wrote
extern "C" int64_t spv_knn_paged_ws_bytes(int32_t n_q, int32_t k, int32_t n_split) {
  if (n_q < 1 || k < 1 || n_split <= 1) return 0;
  return (int64_t)n_split * n_q * (k < KNN_KMAX ? k : KNN_KMAX) * 8;
}

extern "C" int spv_knn_paged(const spv_knn_args* x, void* stream) {
  ScanPlan p;
  int rc = scan_check(x, "spv_knn_paged", knn_splits, p, [&](int n_split) {
    if (!x->idx) return fail(SPV_ERR_ARG, "spv_knn_paged: null idx%s");
    if (!x->dist) return fail(SPV_ERR_ARG, "spv_knn_paged: null dist%s");
    if (x->k < 1 || x->k > KNN_PAGED_KMAX) return fail(SPV_ERR_ARG, "spv_knn_paged: k must lie in [1, 256]%s");
    if (x->ld_out < x->k) return fail(SPV_ERR_ARG, "spv_knn_paged: ld_out < k%s");
    if ((int64_t)x->n_q * x->ld_out > INT32_MAX || x->ld_out > INT32_MAX) return fail(SPV_ERR_ARG, "spv_knn_paged: n_q * ld_out exceeds 2^31 - 1%s");
    if ((int64_t)n_split * x->n_q * (x->k < KNN_KMAX ? x->k : KNN_KMAX) > INT32_MAX)
      return fail(SPV_ERR_ARG, "spv_knn_paged: the workspace (n_split * n_q * min(k, 64) entries) exceeds 2^31 - 1%s");
    return SPV_OK;
  });
  if (rc != SPV_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  for (int page = 0; page * KNN_KMAX < x->k; ++page) {
    const int c0 = page * KNN_KMAX, kp = knn_page_cols(x->k, page);
    const KnnArgs a{x->Q, (long)x->ld_q, x->n_q, x->C, (long)x->ld_c, x->n_c, x->D, kp, x->exclude, p.n_split, p.per,
                    x->idx + c0, x->dist + c0, (int)x->ld_out, (knn_key_t*)x->ws};
    scan_dispatch(a.D, [&](auto dp) {
      constexpr int DP = decltype(dp)::value;
      if (page == 0) launch_lds_upto<knn_partial_kernel<DP>>(p.grid, dim3(KNN_TQ), knn_lds_bytes(DP, KNN_KMAX), knn_lds_bytes(DP, kp), s, a);
      else launch_lds_upto<knn_partial_kernel<DP, true>>(p.grid, dim3(KNN_TQ), knn_lds_bytes(DP, KNN_KMAX), knn_lds_bytes(DP, kp), s, a);
    });
    rc = launch_status(p.n_split == 1 ? "spv_knn_paged" : "spv_knn_paged (partial pass)");
    if (rc != SPV_OK) return rc;
    if (p.n_split == 1) continue;
    hipLaunchKernelGGL(knn_merge_kernel, dim3(p.grid.x), dim3(KNN_TQ), knn_lds_bytes(0, kp), s, a);
    rc = launch_status("spv_knn_paged (merge pass)");
    if (rc != SPV_OK) return rc;
  }
  return SPV_OK;
}

// ---------------------------------------------------------------------------------------------
// LISI on the paged neighbour lists (spv_lisi.h)
// ---------------------------------------------------------------------------------------------
extern "C" int spv_lisi(const spv_lisi_args* x, void* stream) {
  if (!x) return fail(SPV_ERR_ARG, "spv_lisi: null arguments%s");
  if (!x->idx) return fail(SPV_ERR_ARG, "spv_lisi: null idx%s");
  if (!x->dist) return fail(SPV_ERR_ARG, "spv_lisi: null dist%s");
  if (!x->codes) return fail(SPV_ERR_ARG, "spv_lisi: null codes%s");
  if (!x->lisi) return fail(SPV_ERR_ARG, "spv_lisi: null lisi%s");
  if (!x->beta) return fail(SPV_ERR_ARG, "spv_lisi: null beta%s");
  if (!x->n_valid) return fail(SPV_ERR_ARG, "spv_lisi: null n_valid%s");
  if (!x->converged) return fail(SPV_ERR_ARG, "spv_lisi: null converged%s");
  if (x->n < 1) return fail(SPV_ERR_ARG, "spv_lisi: n < 1%s");
  if (x->k < 1 || x->k > LISI_KMAX) return fail(SPV_ERR_ARG, "spv_lisi: k must lie in [1, 256]%s");
  if (x->ld < x->k) return fail(SPV_ERR_ARG, "spv_lisi: ld < k%s");
  if (x->n_c < 0) return fail(SPV_ERR_ARG, "spv_lisi: n_c < 0%s");
  if (x->n_sets < 1 || x->n_sets > LISI_SETS_MAX) return fail(SPV_ERR_ARG, "spv_lisi: n_sets must lie in [1, 8]%s");
  if (!(x->perplexity >= 1.0 && x->perplexity < INFINITY)) return fail(SPV_ERR_ARG, "spv_lisi: perplexity must be a finite number >= 1%s");
  const LisiArgs a{x->idx, x->dist, (long)x->ld, x->n, x->k, x->codes, x->n_c, x->n_sets, log(x->perplexity), x->lisi, x->beta, x->n_valid, x->converged};
  hipLaunchKernelGGL(lisi_kernel, dim3((unsigned)((x->n + LISI_WAVES - 1) / LISI_WAVES)), dim3(LISI_WAVES * LISI_LANES), 0, (hipStream_t)stream, a);
  return launch_status("spv_lisi");
}

// ---------------------------------------------------------------------------------------------
// entropic optimal transport: fused soft-min and top-k over all pairs (spv_ot.h)
// ---------------------------------------------------------------------------------------------
extern "C" int32_t spv_ot_tile_q(void) { return KNN_TQ; }
extern "C" int32_t spv_ot_tile_c(void) { return KNN_TC; }
extern "C" int32_t spv_ot_splits(int32_t n_q, int32_t n_c) { return knn_splits(n_q, n_c); }
extern "C" int64_t spv_ot_ws_bytes(int32_t n_q, int32_t k, int32_t n_split) {
  if (n_q < 1 || k < 0 || n_split <= 1) return 0;
  return (int64_t)n_split * n_q * (k ? k : 1) * 8;
}

// what both entry points refuse, then the kernels' arguments with the resolved chunks; `topk`: the checks of k and the lists
static int ot_check(const spv_ot_args* x, const char* who, bool topk, OtArgs& a, ScanPlan& p) {
  const int rc = scan_check(x, who, knn_splits, p, [&](int n_split) {
    if (!x->h) return fail(SPV_ERR_ARG, "%s: null h", who);
    if (!topk && !x->L) return fail(SPV_ERR_ARG, "%s: null L", who);
    if (topk && !x->r) return fail(SPV_ERR_ARG, "%s: null r", who);
    if (topk && !x->idx) return fail(SPV_ERR_ARG, "%s: null idx", who);
    if (topk && !x->val) return fail(SPV_ERR_ARG, "%s: null val", who);
    if (topk && !x->mass) return fail(SPV_ERR_ARG, "%s: null mass", who);
    if (!(x->inv_eps > 0.f && x->inv_eps < INFINITY)) return fail(SPV_ERR_ARG, "%s: inv_eps must be a positive finite number", who);
    const int rc = topk ? scan_check_rows(x, who) : SPV_OK;
    if (rc != SPV_OK) return rc;
    if ((int64_t)n_split * x->n_q * (topk ? x->k : 1) > INT32_MAX) return fail(SPV_ERR_ARG, "%s: the workspace (n_split * n_q [* k] entries) exceeds 2^31 - 1", who);
    return SPV_OK;
  });
  if (rc != SPV_OK) return rc;
  a = OtArgs{x->Q, (long)x->ld_q, x->n_q, x->C, (long)x->ld_c, x->n_c, x->D, topk ? x->k : 0, x->h, x->r, x->inv_eps, p.n_split,
             p.per, x->L, x->idx, x->val, (long)x->ld_out, x->mass, x->ws};
  return SPV_OK;
}

extern "C" int spv_ot_softmin(const spv_ot_args* x, void* stream) {
  OtArgs a;
  ScanPlan p;
  int rc = ot_check(x, "spv_ot_softmin", false, a, p);
  if (rc != SPV_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  scan_dispatch(a.D, [&](auto dp) { constexpr int DP = decltype(dp)::value; hipLaunchKernelGGL((ot_softmin_kernel<DP>), p.grid, dim3(KNN_TQ), ot_softmin_lds_bytes(DP), s, a); });
  rc = launch_status(a.n_split == 1 ? "spv_ot_softmin" : "spv_ot_softmin (partial pass)");
  if (rc != SPV_OK || a.n_split == 1) return rc;
  hipLaunchKernelGGL(ot_softmin_merge_kernel, dim3(p.grid.x), dim3(KNN_TQ), 0, s, a);
  return launch_status("spv_ot_softmin (merge pass)");
}

extern "C" int spv_ot_topk(const spv_ot_args* x, void* stream) {
  OtArgs a;
  ScanPlan p;
  int rc = ot_check(x, "spv_ot_topk", true, a, p);
  if (rc != SPV_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  // the opt-in is to the largest LDS a call can ask for (k = SPV_OT_KMAX: beyond the 64 KiB a kernel gets unasked), the launch takes what k needs
  scan_dispatch(a.D, [&](auto dp) { constexpr int DP = decltype(dp)::value; launch_lds_upto<ot_topk_kernel<DP>>(p.grid, dim3(KNN_TQ), ot_topk_lds_bytes(DP, KNN_KMAX), ot_topk_lds_bytes(DP, a.k), s, a); });
  rc = launch_status(a.n_split == 1 ? "spv_ot_topk" : "spv_ot_topk (partial pass)");
  if (rc != SPV_OK || a.n_split == 1) return rc;
  hipLaunchKernelGGL(ot_topk_merge_kernel, dim3(p.grid.x), dim3(KNN_TQ), ot_topk_lds_bytes(0, a.k) - ot_tile_words(0) * 4, s, a);   // at most the 64 KiB a kernel gets unasked
  return launch_status("spv_ot_topk (merge pass)");
}

// ---------------------------------------------------------------------------------------------
// the plan's log mass between every query and every segment of the candidates (spv_ot_segments.h)
// ---------------------------------------------------------------------------------------------
extern "C" int32_t spv_ot_segment_splits(int32_t n_q, int32_t n_c) { return otseg_splits(n_q, n_c); }
extern "C" int64_t spv_ot_segment_ws_bytes(int32_t n_q, int32_t n_seg, int32_t n_split) { return otseg_ws_bytes(n_q, n_seg, n_split); }

extern "C" int spv_ot_segment_lse(const spv_ot_seg_args* x, void* stream) {
  ScanPlan p;
  int rc = scan_check(x, "spv_ot_segment_lse", otseg_splits, p, [&](int n_split) {
    if (!x->h) return fail(SPV_ERR_ARG, "spv_ot_segment_lse: null h%s");
    if (!x->seg_ptr) return fail(SPV_ERR_ARG, "spv_ot_segment_lse: null seg_ptr%s");
    if (!x->L) return fail(SPV_ERR_ARG, "spv_ot_segment_lse: null L%s");
    if (!(x->inv_eps > 0.f && x->inv_eps < INFINITY)) return fail(SPV_ERR_ARG, "spv_ot_segment_lse: inv_eps must be a positive finite number%s");
    if (x->n_seg < 1 || x->n_seg > OT_SEG_MAX) return fail(SPV_ERR_ARG, "spv_ot_segment_lse: n_seg must lie in [1, 256]%s");
    if (x->ld_l < x->n_q) return fail(SPV_ERR_ARG, "spv_ot_segment_lse: ld_l < n_q%s");
    if (x->ld_l > INT32_MAX || (int64_t)x->n_seg * x->ld_l > INT32_MAX) return fail(SPV_ERR_ARG, "spv_ot_segment_lse: n_seg * ld_l exceeds 2^31 - 1%s");
    if ((int64_t)n_split * x->n_seg * x->n_q > INT32_MAX) return fail(SPV_ERR_ARG, "spv_ot_segment_lse: the workspace (n_split * n_seg * n_q entries) exceeds 2^31 - 1%s");
    return SPV_OK;
  });
  if (rc != SPV_OK) return rc;
  const OtSegArgs a{x->Q, (long)x->ld_q, x->n_q, x->C, (long)x->ld_c, x->n_c, x->D, x->h, x->inv_eps, x->seg_ptr, x->n_seg, p.n_split, p.per,
                    x->L, (long)x->ld_l, (OtLse*)x->ws};
  hipStream_t s = (hipStream_t)stream;
  scan_dispatch(a.D, [&](auto dp) { constexpr int DP = decltype(dp)::value; hipLaunchKernelGGL((otseg_partial_kernel<DP>), p.grid, dim3(KNN_TQ), ot_softmin_lds_bytes(DP), s, a); });
  rc = launch_status(p.n_split == 1 ? "spv_ot_segment_lse" : "spv_ot_segment_lse (partial pass)");
  if (rc != SPV_OK || p.n_split == 1) return rc;
  hipLaunchKernelGGL(otseg_merge_kernel, dim3(p.grid.x, (unsigned)a.n_seg), dim3(KNN_TQ), 0, s, a);
  return launch_status("spv_ot_segment_lse (merge pass)");
}

// ---------------------------------------------------------------------------------------------
// barycentric projection through the untruncated plan (spv_ot_project.h)
// ---------------------------------------------------------------------------------------------
extern "C" int32_t spv_ot_project_splits(int32_t n_q, int32_t n_c, int32_t n_v) { return otproj_splits(n_q, n_c, n_v); }
extern "C" int64_t spv_ot_project_ws_bytes(int32_t n_q, int32_t n_v, int32_t n_split) { return otproj_ws_bytes(n_q, n_v, n_split); }
extern "C" int32_t spv_ot_project_block(int32_t D) { return D < 1 || D > KNN_DMAX ? 0 : otproj_block(D <= 16 ? 16 : D <= 32 ? 32 : 64); }

extern "C" int spv_ot_project(const spv_ot_proj_args* x, void* stream) {
  ScanPlan p;
  int rc = scan_check(x, "spv_ot_project", [&](int n_q, int n_c) { return otproj_splits(n_q, n_c, x->n_v); }, p, [&](int n_split) {
    if (!x->h) return fail(SPV_ERR_ARG, "spv_ot_project: null h%s");
    if (!x->out) return fail(SPV_ERR_ARG, "spv_ot_project: null out%s");
    if (!x->V && x->n_c > 0) return fail(SPV_ERR_ARG, "spv_ot_project: null V%s");
    if (!(x->inv_eps > 0.f && x->inv_eps < INFINITY)) return fail(SPV_ERR_ARG, "spv_ot_project: inv_eps must be a positive finite number%s");
    if (x->n_v < 1 || x->n_v > OT_VAL_MAX) return fail(SPV_ERR_ARG, "spv_ot_project: n_v must lie in [1, 256]%s");
    if (x->ld_v < x->n_v) return fail(SPV_ERR_ARG, "spv_ot_project: ld_v < n_v%s");
    if (x->ld_out < x->n_q) return fail(SPV_ERR_ARG, "spv_ot_project: ld_out < n_q%s");
    if (x->ld_out > INT32_MAX || (int64_t)x->n_v * x->ld_out > INT32_MAX) return fail(SPV_ERR_ARG, "spv_ot_project: n_v * ld_out exceeds 2^31 - 1%s");
    if (otproj_ws_words(x->n_q, x->n_v, n_split) > INT32_MAX) return fail(SPV_ERR_ARG, "spv_ot_project: the workspace (n_split * (n_v + 2 * blocks) * n_q words) exceeds 2^31 - 1%s");
    return SPV_OK;
  });
  if (rc != SPV_OK) return rc;
  const int VB = spv_ot_project_block(x->D);
  const OtProjArgs a{x->Q, (long)x->ld_q, x->n_q, x->C, (long)x->ld_c, x->n_c, x->D, x->h, x->inv_eps, x->V, (long)x->ld_v, x->n_v, p.n_split, p.per,
                     x->out, (long)x->ld_out, x->L, (float*)x->ws, otproj_ws_rows(x->n_v, VB)};
  p.grid.z = (unsigned)((a.n_v + VB - 1) / VB);
  hipStream_t s = (hipStream_t)stream;
  scan_dispatch(a.D, [&](auto dp) { constexpr int DP = decltype(dp)::value; hipLaunchKernelGGL((otproj_partial_kernel<DP>), p.grid, dim3(KNN_TQ), otproj_lds_bytes(DP), s, a); });
  rc = launch_status(p.n_split == 1 ? "spv_ot_project" : "spv_ot_project (partial pass)");
  if (rc != SPV_OK || p.n_split == 1) return rc;
  hipLaunchKernelGGL(otproj_merge_kernel, dim3(p.grid.x, (unsigned)a.n_v), dim3(KNN_TQ), 0, s, a, VB);
  return launch_status("spv_ot_project (merge pass)");
}

// ---------------------------------------------------------------------------------------------
// segmented distance sums for the silhouette widths (spv_silhouette.h)
// ---------------------------------------------------------------------------------------------
extern "C" int32_t spv_silhouette_splits(int32_t n_q, int32_t n_c) { return sil_splits(n_q, n_c); }
extern "C" int64_t spv_silhouette_ws_bytes(int32_t n_q, int32_t n_seg, int32_t n_split) { return sil_ws_bytes(n_q, n_seg, n_split); }

extern "C" int spv_silhouette_sums(const spv_silhouette_args* x, void* stream) {
  ScanPlan p;
  int rc = scan_check(x, "spv_silhouette_sums", sil_splits, p, [&](int) {
    if (!x->seg_ptr) return fail(SPV_ERR_ARG, "spv_silhouette_sums: null seg_ptr%s");
    if (!x->S) return fail(SPV_ERR_ARG, "spv_silhouette_sums: null S%s");
    if (x->n_seg < 1 || x->n_seg > SIL_SEG_MAX) return fail(SPV_ERR_ARG, "spv_silhouette_sums: n_seg must lie in [1, 256]%s");
    if (x->ld_s < x->n_q) return fail(SPV_ERR_ARG, "spv_silhouette_sums: ld_s < n_q%s");
    return SPV_OK;
  });
  if (rc != SPV_OK) return rc;
  const SilArgs a{x->Q, (long)x->ld_q, x->n_q, x->C, (long)x->ld_c, x->n_c, x->D, x->seg_ptr, x->n_seg, p.n_split, p.per,
                  x->S, (long)x->ld_s, (double*)x->ws};
  hipStream_t s = (hipStream_t)stream;
  scan_dispatch(a.D, [&](auto dp) { constexpr int DP = decltype(dp)::value; hipLaunchKernelGGL((sil_partial_kernel<DP>), p.grid, dim3(KNN_TQ), sil_lds_bytes(DP), s, a); });
  rc = launch_status(p.n_split == 1 ? "spv_silhouette_sums" : "spv_silhouette_sums (partial pass)");
  if (rc != SPV_OK || p.n_split == 1) return rc;
  hipLaunchKernelGGL(sil_merge_kernel, dim3(p.grid.x, (unsigned)a.n_seg), dim3(KNN_TQ), 0, s, a);
  return launch_status("spv_silhouette_sums (merge pass)");
}

// ---------------------------------------------------------------------------------------------
// the fp64 Gram of an fp32 block (spv_gram.h)
// ---------------------------------------------------------------------------------------------
extern "C" int32_t spv_gram_slabs(int32_t n, int32_t n_use) { return gram_slabs(n, n_use); }
extern "C" uint64_t spv_gram_ws_bytes(int32_t n, int32_t n_use) { return (uint64_t)gram_ws_bytes(n, n_use); }

extern "C" int spv_gram_f64(const spv_gram_args* x, void* stream) {
  if (!x) return fail(SPV_ERR_ARG, "spv_gram_f64: null arguments%s");
  if (!x->x) return fail(SPV_ERR_ARG, "spv_gram_f64: null x%s");
  if (!x->sums) return fail(SPV_ERR_ARG, "spv_gram_f64: null sums%s");
  if (!x->gram) return fail(SPV_ERR_ARG, "spv_gram_f64: null gram%s");
  if (x->n < 1 || x->n > GRAM_MAX_N) return fail(SPV_ERR_ARG, "spv_gram_f64: n must lie in [1, 4096]%s");
  if (x->n_rows < 0) return fail(SPV_ERR_ARG, "spv_gram_f64: n_rows < 0%s");
  if (x->rows && x->n_use < 0) return fail(SPV_ERR_ARG, "spv_gram_f64: n_use < 0%s");
  if (x->ld_x < x->n) return fail(SPV_ERR_ARG, "spv_gram_f64: ld_x < n%s");
  if (x->ld_gram < x->n) return fail(SPV_ERR_ARG, "spv_gram_f64: ld_gram < n%s");
  if (reinterpret_cast<uintptr_t>(x->x) & 3) return fail(SPV_ERR_ARG, "spv_gram_f64: x must be 4-byte aligned%s");
  if (reinterpret_cast<uintptr_t>(x->sums) & 7) return fail(SPV_ERR_ARG, "spv_gram_f64: sums must be 8-byte aligned%s");
  if (reinterpret_cast<uintptr_t>(x->gram) & 7) return fail(SPV_ERR_ARG, "spv_gram_f64: gram must be 8-byte aligned%s");
  if (reinterpret_cast<uintptr_t>(x->ws) & 7) return fail(SPV_ERR_ARG, "spv_gram_f64: ws must be 8-byte aligned%s");
  const int n_use = x->rows ? x->n_use : x->n_rows;
  const int slabs = gram_slabs(x->n, n_use);
  const uint64_t need = (uint64_t)gram_ws_doubles(x->n, slabs) * 8;
  if (need && !x->ws) return fail(SPV_ERR_ARG, "spv_gram_f64: null ws%s");
  if (x->ws_bytes < need) return fail(SPV_ERR_ARG, "spv_gram_f64: ws_bytes is less than spv_gram_ws_bytes(n, n_use)%s");
  if (n_use == 0 || x->n_rows == 0) return SPV_OK;   // nothing is counted: nothing changes
  const int nt = gram_tiles(x->n), tiles = gram_tri_tiles(nt);
  const GramArgs a{x->x, (long)x->ld_x, x->n_rows, x->rows, n_use, x->n, x->sums, x->gram, (long)x->ld_gram, (double*)x->ws,
                   slabs, gram_slab_rows(n_use, slabs), nt, tiles};
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(gram_partial_kernel, dim3((unsigned)tiles, (unsigned)slabs), dim3(GRAM_THREADS), 0, s, a);
  int rc = launch_status(slabs == 1 ? "spv_gram_f64" : "spv_gram_f64 (partial pass)");
  if (rc != SPV_OK || slabs == 1) return rc;
  hipLaunchKernelGGL(gram_merge_kernel, dim3((unsigned)tiles, GRAM_T * GRAM_T / GRAM_THREADS), dim3(GRAM_THREADS), 0, s, a);
  return launch_status("spv_gram_f64 (merge pass)");
}

// ---------------------------------------------------------------------------------------------
// rank sums of the observed counts: segmented column sort with tie runs (spv_rank.h)
// ---------------------------------------------------------------------------------------------
extern "C" int32_t spv_rank_gene_slab(void) { return RANK_SLAB; }
extern "C" int32_t spv_rank_lds_capacity(void) { return RANK_LDS_CAP; }
extern "C" int32_t spv_rank_stage_tile(void) { return RANK_TP; }
extern "C" int32_t spv_rank_sort_tile(void) { return RANK_THREADS; }
extern "C" int64_t spv_rank_ws_bytes(int32_t n, int32_t n_sel) { return rank_ws_bytes(n, n_sel); }

// what every entry point of the column sort checks: the list, the slab and the workspace (need: the bytes it takes; values: of the rank transform)
static int rank_list_check(const char* who, int n, int n_sel, const void* ws, int64_t ws_bytes, int64_t need, bool values) {
  if (n_sel < 1 || n_sel > RANK_SLAB) return fail(SPV_ERR_ARG, "%s: n_sel must lie in [1, spv_rank_gene_slab()]", who);
  if (!ws) return fail(SPV_ERR_ARG, "%s: null ws", who);
  if (reinterpret_cast<uintptr_t>(ws) & 7) return fail(SPV_ERR_ARG, "%s: ws must be 8-byte aligned", who);
  if (ws_bytes < need) return fail(SPV_ERR_ARG, values ? "%s: ws_bytes is less than spv_rank_values_ws_bytes(n, n_sel)" : "%s: ws_bytes is less than spv_rank_ws_bytes(n, n_sel)", who);
  return SPV_OK;
}

static int rank_check(const spv_rank_args* x, const char* who) {
  if (!x) return fail(SPV_ERR_ARG, "%s: null arguments", who);
  if (x->n < 1 || x->n > RANK_MAX_N) return fail(SPV_ERR_ARG, "%s: n must lie in [1, 2^20]", who);
  if (x->n_seg < 1 || x->n_seg > RANK_MAX_SEG) return fail(SPV_ERR_ARG, "%s: n_seg must lie in [1, 1024]", who);
  return rank_list_check(who, x->n, x->n_sel, x->ws, x->ws_bytes, rank_ws_bytes(x->n, x->n_sel), false);
}

// what both stage entry points check of the matrix, the piece and the gene slab
static int rank_stage_check(const char* who, const spv_counts& c, int G, int n_rows, int n_piece, int pos_off, int n, int n_sel, const int32_t* genes) {
  if (!c.X) return fail(SPV_ERR_ARG, "%s: null count matrix", who);
  if (c.dtype != SPV_COUNT_U16 && c.dtype != SPV_COUNT_F32) return fail(SPV_ERR_ARG, "%s: unknown count dtype", who);
  if (G <= 0 || n_rows <= 0) return fail(SPV_ERR_ARG, "%s: G and n_rows must be positive", who);
  if (n_piece <= 0 || pos_off < 0 || (int64_t)pos_off + n_piece > n) return fail(SPV_ERR_ARG, "%s: the piece [pos_off, pos_off + n_piece) must be non-empty and lie in [0, n)", who);
  if (!c.rows && n_piece > n_rows) return fail(SPV_ERR_ARG, "%s: without a row list n_piece must not exceed n_rows", who);
  if (c.col_off < 0 || c.ld < (int64_t)c.col_off + G) return fail(SPV_ERR_ARG, "%s: ld < col_off + G", who);
  if (!genes && n_sel > G) return fail(SPV_ERR_ARG, "%s: without a gene list n_sel must not exceed G", who);
  return SPV_OK;
}

// the stage's launches: the reset of the head when asked for, then the tiles of the piece
template <bool POS>
static int rank_stage_launch(const char* who, const char* who_reset, const RankArgs& a, bool u16, bool reset, hipStream_t s) {
  if (reset) {
    hipLaunchKernelGGL(rank_reset_kernel, dim3((RANK_SLAB + RANK_MAX_SEG) / 256), dim3(256), 0, s, (int*)a.ws);
    const int rc = launch_status(who_reset);
    if (rc != SPV_OK) return rc;
  }
  const dim3 grid((unsigned)((a.n_piece + RANK_TP - 1) / RANK_TP), (unsigned)((a.n_sel + RANK_TG - 1) / RANK_TG));
  if (u16) hipLaunchKernelGGL((rank_stage_kernel<true, POS>), grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((rank_stage_kernel<false, POS>), grid, dim3(256), 0, s, a);
  return launch_status(who);
}

static RankArgs rank_args(const spv_rank_args* x) {
  return RankArgs{x->x.X, (long)x->x.ld, x->x.rows, x->x.col_off, x->G, x->n_rows, x->n_piece, x->pos_off, x->n, x->n_seg, x->n_sel,
                  x->seg, x->w, x->genes, (long long*)x->rank2, (long)x->ld_rank2, (long long*)x->ties, (char*)x->ws};
}

extern "C" int spv_rank_stage(const spv_rank_args* x, void* stream) {
  const char* const who = "spv_rank_stage";
  int rc = rank_check(x, who);
  if (rc != SPV_OK) return rc;
  if (!x->seg && x->x.X) return fail(SPV_ERR_ARG, "%s: null seg", who);   // (a null matrix is reported first, as before the checks were shared)
  rc = rank_stage_check(who, x->x, x->G, x->n_rows, x->n_piece, x->pos_off, x->n, x->n_sel, x->genes);
  if (rc != SPV_OK) return rc;
  return rank_stage_launch<false>(who, "spv_rank_stage (reset)", rank_args(x), x->x.dtype == SPV_COUNT_U16, x->reset != 0, (hipStream_t)stream);
}

extern "C" int spv_rank_sums(const spv_rank_args* x, void* stream) {
  const char* const who = "spv_rank_sums";
  int rc = rank_check(x, who);
  if (rc != SPV_OK) return rc;
  if (!x->rank2) return fail(SPV_ERR_ARG, "%s: null rank2", who);
  if (!x->ties) return fail(SPV_ERR_ARG, "%s: null ties", who);
  if (x->ld_rank2 < x->n_sel) return fail(SPV_ERR_ARG, "%s: ld_rank2 < n_sel", who);
  if (reinterpret_cast<uintptr_t>(x->rank2) & 7) return fail(SPV_ERR_ARG, "%s: rank2 must be 8-byte aligned", who);
  if (reinterpret_cast<uintptr_t>(x->ties) & 7) return fail(SPV_ERR_ARG, "%s: ties must be 8-byte aligned", who);
  const RankArgs a = rank_args(x);
  hipLaunchKernelGGL(rank_sums_kernel, dim3((unsigned)x->n_sel), dim3(RANK_THREADS), 0, (hipStream_t)stream, a);
  return launch_status(who);
}

// ---------------------------------------------------------------------------------------------
// the rank transform on the same column sort (spv_rank_values.h)
// ---------------------------------------------------------------------------------------------
extern "C" int64_t spv_rank_values_ws_bytes(int32_t n, int32_t n_sel) { return rank_values_ws_bytes(n, n_sel); }

static int rank_values_check(const spv_rank_values_args* x, const char* who) {
  if (!x) return fail(SPV_ERR_ARG, "%s: null arguments", who);
  if (x->n < 1 || x->n > RANK_MAX_N) return fail(SPV_ERR_ARG, "%s: n must lie in [1, 2^20]", who);
  return rank_list_check(who, x->n, x->n_sel, x->ws, x->ws_bytes, rank_values_ws_bytes(x->n, x->n_sel), true);
}

extern "C" int spv_rank_values_stage(const spv_rank_values_args* x, void* stream) {
  const char* const who = "spv_rank_values_stage";
  int rc = rank_values_check(x, who);
  if (rc != SPV_OK) return rc;
  rc = rank_stage_check(who, x->x, x->G, x->n_rows, x->n_piece, x->pos_off, x->n, x->n_sel, x->genes);
  if (rc != SPV_OK) return rc;
  const RankArgs a{x->x.X, (long)x->x.ld, x->x.rows, x->x.col_off, x->G, x->n_rows, x->n_piece, x->pos_off, x->n, 0, x->n_sel,
                   nullptr, x->w, x->genes, nullptr, 0, nullptr, (char*)x->ws};
  return rank_stage_launch<true>(who, "spv_rank_values_stage (reset)", a, x->x.dtype == SPV_COUNT_U16, x->reset != 0, (hipStream_t)stream);
}

extern "C" int spv_rank_values(const spv_rank_values_args* x, void* stream) {
  const char* const who = "spv_rank_values";
  int rc = rank_values_check(x, who);
  if (rc != SPV_OK) return rc;
  if (!x->out) return fail(SPV_ERR_ARG, "%s: null out", who);
  if (x->ld_out < x->n_sel) return fail(SPV_ERR_ARG, "%s: ld_out < n_sel", who);
  if (reinterpret_cast<uintptr_t>(x->out) & 3) return fail(SPV_ERR_ARG, "%s: out must be 4-byte aligned", who);
  if (reinterpret_cast<uintptr_t>(x->ties) & 7) return fail(SPV_ERR_ARG, "%s: ties must be 8-byte aligned", who);
  if (reinterpret_cast<uintptr_t>(x->nonzero) & 3) return fail(SPV_ERR_ARG, "%s: nonzero must be 4-byte aligned", who);
  const RankValuesArgs a{x->n, x->n_sel, x->out, (long)x->ld_out, (long long*)x->ties, x->nonzero, (char*)x->ws};
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(rank_values_kernel, dim3((unsigned)x->n_sel), dim3(RANK_THREADS), 0, s, a);
  rc = launch_status("spv_rank_values (walk)");
  if (rc != SPV_OK) return rc;
  hipLaunchKernelGGL(rank_values_store_kernel, dim3((unsigned)((x->n + RANKV_T - 1) / RANKV_T), (unsigned)((x->n_sel + RANKV_T - 1) / RANKV_T)), dim3(RANKV_THREADS), 0, s, a);
  return launch_status(who);
}

// ---------------------------------------------------------------------------------------------
// PCA of the log-normalised counts: the operand stage and the two skinny products on the fp32 MFMA (spv_pca.h)
// ---------------------------------------------------------------------------------------------
extern "C" int32_t spv_pca_slab(void) { return PCA_SLAB; }
extern "C" int32_t spv_pca_cell_tile(void) { return PCA_CELL_TILE; }
extern "C" int64_t spv_pca_ws_bytes(int32_t G, int32_t n_piece, int32_t l) { return pca_ws_bytes(G, n_piece, l); }

// what the three entry points check of the matrix, the list and the piece
static int pca_check(const spv_pca_args* x, const char* who) {
  if (!x) return fail(SPV_ERR_ARG, "%s: null arguments", who);
  if (!x->x.X) return fail(SPV_ERR_ARG, "%s: null count matrix", who);
  if (x->x.dtype != SPV_COUNT_U16 && x->x.dtype != SPV_COUNT_F32) return fail(SPV_ERR_ARG, "%s: unknown count dtype", who);
  if (x->G < 1 || x->n_rows < 1) return fail(SPV_ERR_ARG, "%s: G and n_rows must be positive", who);
  if (x->n < 1) return fail(SPV_ERR_ARG, "%s: n < 1", who);
  if (x->n_piece < 1 || x->pos_off < 0 || (int64_t)x->pos_off + x->n_piece > x->n) return fail(SPV_ERR_ARG, "%s: the piece [pos_off, pos_off + n_piece) must be non-empty and lie in [0, n)", who);
  if (!x->x.rows && x->n_piece > x->n_rows) return fail(SPV_ERR_ARG, "%s: without a row list n_piece must not exceed n_rows", who);
  if (x->x.col_off < 0 || x->x.ld < (int64_t)x->x.col_off + x->G) return fail(SPV_ERR_ARG, "%s: ld < col_off + G", who);
  return SPV_OK;
}
// ... and of the l columns of the two products
static int pca_check_y(const spv_pca_args* x, const char* who) {
  if (!pca_l_ok(x->l)) return fail(SPV_ERR_ARG, "%s: l must be 16, 32, 48 or 64", who);
  if (!x->Y) return fail(SPV_ERR_ARG, "%s: null Y", who);
  if (x->ld_y < x->l) return fail(SPV_ERR_ARG, "%s: ld_y < l", who);
  return SPV_OK;
}

static PcaArgs pca_args(const spv_pca_args* x) {
  return PcaArgs{x->x.X, (long)x->x.ld, x->x.rows, x->x.col_off, x->G, x->n_rows, x->n_piece, x->pos_off, x->n, x->l, x->w, x->mu, x->scale,
                 x->block, (long)x->ld_block, x->V, (long)x->ld_v, x->Y, (long)x->ld_y, x->Z, (long)x->ld_z, (float*)x->ws};
}

extern "C" int spv_pca_stage(const spv_pca_args* x, void* stream) {
  const char* const who = "spv_pca_stage";
  int rc = pca_check(x, who);
  if (rc != SPV_OK) return rc;
  if (!x->block) return fail(SPV_ERR_ARG, "%s: null block", who);
  if (x->ld_block < x->G) return fail(SPV_ERR_ARG, "%s: ld_block < G", who);
  const PcaArgs a = pca_args(x);
  const dim3 grid((unsigned)((x->n_piece + PCA_ST_P - 1) / PCA_ST_P), (unsigned)((x->G + PCA_THREADS - 1) / PCA_THREADS));
  if (x->x.dtype == SPV_COUNT_U16) hipLaunchKernelGGL(pca_stage_kernel<true>, grid, dim3(PCA_THREADS), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(pca_stage_kernel<false>, grid, dim3(PCA_THREADS), 0, (hipStream_t)stream, a);
  return launch_status(who);
}

extern "C" int spv_pca_project(const spv_pca_args* x, void* stream) {
  const char* const who = "spv_pca_project";
  int rc = pca_check(x, who);
  if (rc == SPV_OK) rc = pca_check_y(x, who);
  if (rc != SPV_OK) return rc;
  if (!x->V) return fail(SPV_ERR_ARG, "%s: null V", who);
  if (x->ld_v < x->l) return fail(SPV_ERR_ARG, "%s: ld_v < l", who);
  const PcaArgs a = pca_args(x);
  const dim3 grid((unsigned)((x->n_piece + PCA_CELL_TILE - 1) / PCA_CELL_TILE));
  if (x->x.dtype == SPV_COUNT_U16) hipLaunchKernelGGL(pca_project_kernel<true>, grid, dim3(PCA_THREADS), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(pca_project_kernel<false>, grid, dim3(PCA_THREADS), 0, (hipStream_t)stream, a);
  return launch_status(who);
}

extern "C" int spv_pca_back(const spv_pca_args* x, void* stream) {
  const char* const who = "spv_pca_back";
  int rc = pca_check(x, who);
  if (rc == SPV_OK) rc = pca_check_y(x, who);
  if (rc != SPV_OK) return rc;
  if (x->pos_off % PCA_SLAB) return fail(SPV_ERR_ARG, "%s: pos_off must be a multiple of spv_pca_slab()", who);
  if (!x->Z) return fail(SPV_ERR_ARG, "%s: null Z", who);
  if (reinterpret_cast<uintptr_t>(x->Z) & 7) return fail(SPV_ERR_ARG, "%s: Z must be 8-byte aligned", who);
  if (x->ld_z < x->l) return fail(SPV_ERR_ARG, "%s: ld_z < l", who);
  if (!x->ws) return fail(SPV_ERR_ARG, "%s: null ws", who);
  if (reinterpret_cast<uintptr_t>(x->ws) & 7) return fail(SPV_ERR_ARG, "%s: ws must be 8-byte aligned", who);
  if (x->ws_bytes < pca_ws_bytes(x->G, x->n_piece, x->l)) return fail(SPV_ERR_ARG, "%s: ws_bytes is less than spv_pca_ws_bytes(G, n_piece, l)", who);
  const PcaArgs a = pca_args(x);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)(pca_gene_pad(x->G) / PCA_GENE_TILE), (unsigned)pca_slabs(x->n_piece));
  if (x->x.dtype == SPV_COUNT_U16) hipLaunchKernelGGL(pca_back_kernel<true>, grid, dim3(PCA_THREADS), 0, s, a);
  else hipLaunchKernelGGL(pca_back_kernel<false>, grid, dim3(PCA_THREADS), 0, s, a);
  rc = launch_status("spv_pca_back (partial pass)");
  if (rc != SPV_OK) return rc;
  hipLaunchKernelGGL(pca_merge_kernel, dim3((unsigned)(((long)x->G * x->l + PCA_THREADS - 1) / PCA_THREADS)), dim3(PCA_THREADS), 0, s, a);
  return launch_status("spv_pca_back (merge pass)");
}

// ---------------------------------------------------------------------------------------------
// exact t-SNE: the all-pairs half, the perplexity calibration, the sparse half with the step (spv_tsne.h)
// ---------------------------------------------------------------------------------------------
extern "C" int32_t spv_tsne_splits(int32_t n_q, int32_t n_c) { return tsne_splits(n_q, n_c); }
extern "C" int64_t spv_tsne_ws_bytes(int32_t n_q, int32_t D, int32_t n_split) { return tsne_ws_bytes(n_q, D, n_split); }

extern "C" int spv_tsne_repulsion(const spv_tsne_rep_args* x, void* stream) {
  ScanPlan p;
  int rc = scan_check(x, "spv_tsne_repulsion", tsne_splits, p, [&](int) {
    if (x->D > TSNE_DMAX) return fail(SPV_ERR_ARG, "spv_tsne_repulsion: D must lie in [1, 4]%s");
    if (!x->Zrow) return fail(SPV_ERR_ARG, "spv_tsne_repulsion: null Zrow%s");
    if (!x->F) return fail(SPV_ERR_ARG, "spv_tsne_repulsion: null F%s");
    if (x->ld_f < x->n_q) return fail(SPV_ERR_ARG, "spv_tsne_repulsion: ld_f < n_q%s");
    return SPV_OK;
  });
  if (rc != SPV_OK) return rc;
  const TsneArgs a{x->Q, (long)x->ld_q, x->n_q, x->C, (long)x->ld_c, x->n_c, x->D, x->exclude, p.n_split, p.per, x->Zrow, x->F, (long)x->ld_f,
                   (double*)x->ws};
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(tsne_partial_kernel, p.grid, dim3(KNN_TQ), 0, s, a);
  rc = launch_status(p.n_split == 1 ? "spv_tsne_repulsion" : "spv_tsne_repulsion (partial pass)");
  if (rc != SPV_OK || p.n_split == 1) return rc;
  hipLaunchKernelGGL(tsne_merge_kernel, dim3(p.grid.x, (unsigned)(1 + a.D)), dim3(KNN_TQ), 0, s, a);
  return launch_status("spv_tsne_repulsion (merge pass)");
}

extern "C" int spv_tsne_affinities(const float* d2, float* P, int64_t ld, int32_t n, int32_t k, double perplexity, double* beta, void* stream) {
  if (!d2) return fail(SPV_ERR_ARG, "spv_tsne_affinities: null d2%s");
  if (!P) return fail(SPV_ERR_ARG, "spv_tsne_affinities: null P%s");
  if (!beta) return fail(SPV_ERR_ARG, "spv_tsne_affinities: null beta%s");
  if (n < 1) return fail(SPV_ERR_ARG, "spv_tsne_affinities: n < 1%s");
  if (k < 1 || k > KNN_KMAX) return fail(SPV_ERR_ARG, "spv_tsne_affinities: k must lie in [1, 64]%s");
  if (ld < k) return fail(SPV_ERR_ARG, "spv_tsne_affinities: ld < k%s");
  if (!(perplexity >= 1.0 && perplexity < INFINITY)) return fail(SPV_ERR_ARG, "spv_tsne_affinities: perplexity must be a finite number >= 1%s");
  const TsneAffArgs a{d2, P, (long)ld, n, k, log(perplexity), beta};
  hipLaunchKernelGGL(tsne_affinities_kernel, dim3((unsigned)((n + 127) / 128)), dim3(128), 0, (hipStream_t)stream, a);
  return launch_status("spv_tsne_affinities");
}

extern "C" int spv_tsne_update(const spv_tsne_upd_args* x, void* stream) {
  if (!x) return fail(SPV_ERR_ARG, "spv_tsne_update: null arguments%s");
  if (!x->y_in) return fail(SPV_ERR_ARG, "spv_tsne_update: null y_in%s");
  if (!x->y_out) return fail(SPV_ERR_ARG, "spv_tsne_update: null y_out%s");
  if (!x->indptr) return fail(SPV_ERR_ARG, "spv_tsne_update: null indptr%s");
  if (!x->cols) return fail(SPV_ERR_ARG, "spv_tsne_update: null cols%s");
  if (!x->vals) return fail(SPV_ERR_ARG, "spv_tsne_update: null vals%s");
  if (!x->Zrow) return fail(SPV_ERR_ARG, "spv_tsne_update: null Zrow%s");
  if (!x->F) return fail(SPV_ERR_ARG, "spv_tsne_update: null F%s");
  if (!x->Z) return fail(SPV_ERR_ARG, "spv_tsne_update: null Z%s");
  if (!x->u) return fail(SPV_ERR_ARG, "spv_tsne_update: null u%s");
  if (!x->gain) return fail(SPV_ERR_ARG, "spv_tsne_update: null gain%s");
  if (x->y_out == x->y_in) return fail(SPV_ERR_ARG, "spv_tsne_update: y_out must not be y_in%s");
  if (x->n < 1) return fail(SPV_ERR_ARG, "spv_tsne_update: n < 1%s");
  if (x->D < 1 || x->D > TSNE_DMAX) return fail(SPV_ERR_ARG, "spv_tsne_update: D must lie in [1, 4]%s");
  if (x->ld_y < x->D) return fail(SPV_ERR_ARG, "spv_tsne_update: ld_y < D%s");
  if (x->ld_f < x->n) return fail(SPV_ERR_ARG, "spv_tsne_update: ld_f < n%s");
  for (const double v : {x->alpha, x->momentum, x->lr, x->min_gain})
    if (!(v >= 0.0 && v < INFINITY)) return fail(SPV_ERR_ARG, "spv_tsne_update: alpha, momentum, lr and min_gain must be finite and not negative%s");
  const TsneUpdArgs a{x->y_in, x->y_out, (long)x->ld_y, x->n, x->D, (const long*)x->indptr, x->cols, x->vals, x->Zrow, x->F, (long)x->ld_f, x->Z,
                      x->u, x->gain, x->alpha, x->momentum, x->lr, x->min_gain, x->kl_row, x->grad};
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(tsne_zsum_kernel, dim3(1), dim3(TSNE_ZSUM_T), 0, s, a);
  const int rc = launch_status("spv_tsne_update (sum of Zrow)");
  if (rc != SPV_OK) return rc;
  hipLaunchKernelGGL(tsne_update_kernel, dim3((unsigned)((a.n + 127) / 128)), dim3(128), 0, s, a);
  return launch_status("spv_tsne_update");
}

extern "C" int spv_count_totals(const spv_counts* x, int32_t n_cells, int32_t G, double* total, void* stream) {
  if (!x || !x->X || !total) return fail(SPV_ERR_ARG, "spv_count_totals: null pointer%s");
  if (n_cells <= 0 || G <= 0 || x->col_off < 0 || x->ld < (int64_t)x->col_off + G) return fail(SPV_ERR_ARG, "spv_count_totals: bad shape%s");
  const dim3 grid((unsigned)((n_cells + 3) / 4)), block(256);
  if (x->dtype == SPV_COUNT_U16) hipLaunchKernelGGL((count_totals_kernel<true>), grid, block, 0, (hipStream_t)stream, x->X, (long)x->ld, x->col_off, n_cells, G, total);
  else if (x->dtype == SPV_COUNT_F32) hipLaunchKernelGGL((count_totals_kernel<false>), grid, block, 0, (hipStream_t)stream, x->X, (long)x->ld, x->col_off, n_cells, G, total);
  else return fail(SPV_ERR_ARG, "spv_count_totals: unknown count dtype%s");
  return launch_status("spv_count_totals");
}

extern "C" int spv_csr_totals(const int64_t* indptr, const int32_t* cols, const void* vals, int32_t dtype, int32_t n_cells, int32_t G, double* total, void* stream) {
  if (!indptr || !total || n_cells <= 0 || G <= 0) return fail(SPV_ERR_ARG, "spv_csr_totals: bad arguments%s");
  const dim3 grid((unsigned)((n_cells + 3) / 4)), block(256);
  if (dtype == SPV_COUNT_U16) hipLaunchKernelGGL((csr_totals_kernel<true>), grid, block, 0, (hipStream_t)stream, (const long*)indptr, cols, vals, n_cells, G, total);
  else if (dtype == SPV_COUNT_F32) hipLaunchKernelGGL((csr_totals_kernel<false>), grid, block, 0, (hipStream_t)stream, (const long*)indptr, cols, vals, n_cells, G, total);
  else return fail(SPV_ERR_ARG, "spv_csr_totals: unknown count dtype%s");
  return launch_status("spv_csr_totals");
}

extern "C" int spv_dec_dz(const spv_dec_params* q, const float* Tp, const float* Ts, float* dz_part, void* stream) {
  DecParams p;
  int rc = to_dec(q, p);
  if (rc != SPV_OK) return rc;
  if (!Tp || !Ts || !p.tP || !p.tS || !p.lse_p || !p.lse_s || !dz_part) return fail(SPV_ERR_ARG, "spv_dec_dz: null pointer%s");
  if (p.n_gene_tiles != p.Gp / 32) return fail(SPV_ERR_ARG, "spv_dec_dz: n_gene_tiles must be Gp / 32%s");
  if (p.grads_f32) return fail(SPV_ERR_UNSUPPORTED, "spv_dec_dz: needs bf16 gradient arrays%s");
  if (dec_kw(q) != 1) return fail(SPV_ERR_UNSUPPORTED, "spv_dec_dz: narrow operand layout only (kslots = 0)%s");
  hipLaunchKernelGGL((dec_softmax_bwd_kernel<bf16_t, true, false>), dim3(p.Bp / DEC_CELLS_PER_WG, p.gene_splits), dim3(256), 0, (hipStream_t)stream, p, Tp, Ts, dz_part, (float*)nullptr, (float*)nullptr);
  return launch_status("spv_dec_dz");
}

extern "C" int spv_dec_softmax_bwd(const spv_dec_params* q, const float* Tp, const float* Ts, float* dz_part, void* stream) {
  DecParams p;
  int rc = to_dec(q, p);
  if (rc != SPV_OK) return rc;
  if (!Tp || !Ts || !p.tP || !p.tS || !p.lse_p || !p.lse_s) return fail(SPV_ERR_ARG, "spv_dec_softmax_bwd: null pointer%s");
  if (p.n_gene_tiles != p.Gp / 32) return fail(SPV_ERR_ARG, "spv_dec_softmax_bwd: n_gene_tiles must be Gp / 32%s");
  dim3 grid(p.Bp / DEC_CELLS_PER_WG, p.gene_splits);
  hipStream_t s = (hipStream_t)stream;
  float* const none = nullptr;
  if (dec_kw(q) == 2) {   // wide layout: the in-place fix only (the latent gradient of the rate heads then comes from split-K GEMMs)
    if (dz_part) return fail(SPV_ERR_UNSUPPORTED, "spv_dec_softmax_bwd: the wide operand layout (kslots = 1) takes no dz_part%s");
    if (p.grads_f32) hipLaunchKernelGGL((dec_softmax_bwd_kernel<split_t, false, true, false, 2>), grid, dim3(256), 0, s, p, Tp, Ts, none, none, none);
    else hipLaunchKernelGGL((dec_softmax_bwd_kernel<bf16_t, false, true, false, 2>), grid, dim3(256), 0, s, p, Tp, Ts, none, none, none);
    return launch_status("spv_dec_softmax_bwd");
  }
  if (p.grads_f32 && dz_part) hipLaunchKernelGGL((dec_softmax_bwd_kernel<split_t, true>), grid, dim3(256), 0, s, p, Tp, Ts, dz_part, none, none);
  else if (p.grads_f32) hipLaunchKernelGGL((dec_softmax_bwd_kernel<split_t, false>), grid, dim3(256), 0, s, p, Tp, Ts, none, none, none);
  else if (dz_part) hipLaunchKernelGGL((dec_softmax_bwd_kernel<bf16_t, true>), grid, dim3(256), 0, s, p, Tp, Ts, dz_part, none, none);
  else hipLaunchKernelGGL((dec_softmax_bwd_kernel<bf16_t, false>), grid, dim3(256), 0, s, p, Tp, Ts, none, none, none);
  return launch_status("spv_dec_softmax_bwd");
}

// One read-only pass over t_P / t_S (bf16 gradient arrays) for everything the backward pass needs from them: the latent gradient of the
// two rate heads (dz_part, as spv_dec_softmax_bwd) AND the two regressor weight gradients as per-workgroup-row partial slabs
// dw_part [Bp / 128][Gp][48] = [d W'_p (16 columns) | d W'_s (32 columns)] (sum the first G rows with spv_reduce_slabs).  t_P / t_S are left uncorrected: nothing reads
// them afterwards.  Replaces spv_dec_softmax_bwd + spv_dec_heads_wgrad in bf16 mode.
static int heads_bwd_prepare(const spv_dec_params* q, const float* Tp, const float* Ts, const float* dz_part, const float* dw_part, DecParams& p) {
  int rc = to_dec(q, p);
  if (rc != SPV_OK) return rc;
  if (!Tp || !Ts || !p.tP || !p.tS || !p.lse_p || !p.lse_s || !dz_part || !dw_part) return fail(SPV_ERR_ARG, "spv_dec_heads_bwd: null pointer%s");
  if (p.n_gene_tiles != p.Gp / 32) return fail(SPV_ERR_ARG, "spv_dec_heads_bwd: n_gene_tiles must be Gp / 32%s");
  if (p.Bp % DEC_CELLS_PER_WG) return fail(SPV_ERR_ARG, "spv_dec_heads_bwd: Bp must be a multiple of 128%s");
  if (p.grads_f32 && (!p.Wps_lo || !p.Aps_lo)) return fail(SPV_ERR_ARG, "spv_dec_heads_bwd: split gradient words need the lo planes of the operand images%s");
  if (dec_kw(q) != 1) return fail(SPV_ERR_UNSUPPORTED, "spv_dec_heads_bwd: narrow operand layout only (kslots = 0)%s");
  return SPV_OK;
}
extern "C" int spv_dec_heads_bwd(const spv_dec_params* q, const float* Tp, const float* Ts, float* dz_part, float* dw_part, void* stream) {
  DecParams p;
  int rc = heads_bwd_prepare(q, Tp, Ts, dz_part, dw_part, p);
  if (rc != SPV_OK) return rc;
  dim3 grid(p.Bp / DEC_CELLS_PER_WG, p.gene_splits);
  if (p.grads_f32) {   // hi / lo planes of split-bf16 gradient words ("fp32" mode)
    launch_lds<dec_heads_bwd_split_kernel>(grid, dim3(256), HBS_LDS_BYTES, (hipStream_t)stream, p, Tp, Ts, dz_part, dw_part);
    return launch_status("spv_dec_heads_bwd");
  }
  // (the partial slabs cover gene rows the splits do not reach only when genes_per_split * gene_splits < round_up(G, 32): the host sizes
  // the splits to cover; rows in [round_up(G, 32), Gp) are never written and never read)
  hipLaunchKernelGGL(dec_heads_bwd_kernel, grid, dim3(256), 0, (hipStream_t)stream, p, Tp, Ts, dz_part, dw_part);
  return launch_status("spv_dec_heads_bwd");
}
extern "C" int spv_dec_heads_bwd_grouped(const spv_dec_group* g, int32_t n, void* stream) {
  if (!g || n <= 0) return fail(SPV_ERR_ARG, "spv_dec_heads_bwd_grouped: bad arguments%s");
  return pairs_then_rest(n,
    [&](int i) {
      HeadsBwdArgs a0, a1;
      int rc = heads_bwd_prepare(&g[i].p, g[i].Tp, g[i].Ts, g[i].dz_part, g[i].dw_part, a0.p);
      if (rc != SPV_OK) return rc;
      rc = heads_bwd_prepare(&g[i + 1].p, g[i + 1].Tp, g[i + 1].Ts, g[i + 1].dz_part, g[i + 1].dw_part, a1.p);
      if (rc != SPV_OK) return rc;
      if (a0.p.grads_f32 || a1.p.grads_f32) return NOT_A_PAIR;   // (the split-word kernel takes a whole CU's LDS: no pair form)
      a0.Tp = g[i].Tp; a0.Ts = g[i].Ts; a0.dz_part = g[i].dz_part; a0.dw_part = g[i].dw_part;
      a1.Tp = g[i + 1].Tp; a1.Ts = g[i + 1].Ts; a1.dz_part = g[i + 1].dz_part; a1.dw_part = g[i + 1].dw_part;
      hipLaunchKernelGGL(dec_heads_bwd_pair_kernel, dim3(max2(a0.p.Bp, a1.p.Bp) / DEC_CELLS_PER_WG, max2(a0.p.gene_splits, a1.p.gene_splits), 2), dim3(256), 0, (hipStream_t)stream, a0, a1);
      return launch_status("spv_dec_heads_bwd_grouped");
    },
    [&](int i) { return spv_dec_heads_bwd(&g[i].p, g[i].Tp, g[i].Ts, g[i].dz_part, g[i].dw_part, stream); });
}

// ---------------------------------------------------------------------------------------------
// optimiser: Adam over one flat fp32 parameter buffer (scvi TrainingPlan defaults are passed by the
// host: lr 1e-3, eps 0.01, weight_decay 1e-6 -- training_mixin.py:111).  torch.optim.Adam semantics.
// ---------------------------------------------------------------------------------------------
__global__ void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                            long n, float lr, float b1, float b2, float eps, float wd, float bc1, float bc2, float gscale) {
  const long stride = (long)gridDim.x * blockDim.x * 4;
  const AdamStep a = adam_prologue(lr, b1, b2, eps, wd, bc1, bc2, gscale, nullptr, 0.0, 0.0);
  for (long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += stride) {
    if (i + 4 <= n) {
      f4v pp = *reinterpret_cast<f4v*>(p + i), gg = *reinterpret_cast<const f4v*>(g + i);
      f4v mm = *reinterpret_cast<f4v*>(m + i), vv = *reinterpret_cast<f4v*>(v + i);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float pj = pp[j], mj = mm[j], vj = vv[j];
        adam_update(pj, gg[j], mj, vj, a);
        pp[j] = pj; mm[j] = mj; vv[j] = vj;
      }
      *reinterpret_cast<f4v*>(p + i) = pp; *reinterpret_cast<f4v*>(m + i) = mm; *reinterpret_cast<f4v*>(v + i) = vv;
    } else {
      for (long k = i; k < n; ++k) adam_update(p[k], g[k], m[k], v[k], a);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// several small gathers / copies of 4-byte words in one launch: dst[i] = src[idx ? idx[i] : i].  The step's prologue (two row-index
// copies into the graph's static buffers, two label gathers) is a chain of 5-us launches at the head of the critical path.
// ---------------------------------------------------------------------------------------------
struct GatherBatch { int n; spv_gather_prob p[SPV_MAXP]; };
__global__ __launch_bounds__(256) void gather_u32_kernel(GatherBatch a) {
  const spv_gather_prob& q = a.p[blockIdx.y];
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < q.count) q.dst[i] = q.src[q.idx ? (long)q.idx[i] : i];
}
extern "C" int spv_gather_u32(const spv_gather_prob* probs, int32_t nprob, void* stream) {
  if (!probs || nprob <= 0 || nprob > SPV_MAXP) return fail(SPV_ERR_ARG, "spv_gather_u32: bad arguments%s");
  GatherBatch a{};
  a.n = nprob;
  long nmax = 0;
  for (int i = 0; i < nprob; ++i) {
    if (!probs[i].src || !probs[i].dst || probs[i].count < 0) return fail(SPV_ERR_ARG, "spv_gather_u32: bad problem%s");
    a.p[i] = probs[i];
    nmax = probs[i].count > nmax ? probs[i].count : nmax;
  }
  if (nmax == 0) return SPV_OK;
  hipLaunchKernelGGL(gather_u32_kernel, dim3((unsigned)((nmax + 255) / 256), nprob), dim3(256), 0, (hipStream_t)stream, a);
  return launch_status("spv_gather_u32");
}

// ---------------------------------------------------------------------------------------------
// standard-normal draws from a counter-based generator (Philox 4x32-10 + Box-Muller), keyed by (key, *counter): the step's noise
// comes out of ONE launch that reads a device-resident step counter, so a captured hipGraph needs no generator state from the host
// (torch's graph-safe generator costs two fill launches per replay + its own kernel, at the head of the step's critical path).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void randn_kernel(float* __restrict__ out, long n, const long long* __restrict__ counter, unsigned long long key) {
  const long i4 = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i4 >= n) return;
  const unsigned long long step = counter ? (unsigned long long)*counter : 0ull;
  unsigned c[4] = {(unsigned)(i4 >> 2), (unsigned)((unsigned long long)(i4 >> 2) >> 32), (unsigned)step, (unsigned)(step >> 32)};
  const unsigned k[2] = {(unsigned)key, (unsigned)(key >> 32)};
  philox4x32_10(c, k);
  float z[4];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const float u1 = ((float)(c[2 * h] >> 8) + 0.5f) * (1.0f / 16777216.0f);      // (0, 1)
    const float u2 = ((float)(c[2 * h + 1] >> 8) + 0.5f) * (1.0f / 16777216.0f);
    const float rad = sqrtf(-2.0f * __logf(u1));
    float sn, cs;
    __sincosf(6.283185307179586f * u2, &sn, &cs);
    z[2 * h] = rad * cs; z[2 * h + 1] = rad * sn;
  }
  if (i4 + 4 <= n && ((reinterpret_cast<uintptr_t>(out + i4) & 15) == 0)) *reinterpret_cast<f4v*>(out + i4) = f4v{z[0], z[1], z[2], z[3]};
  else for (int j = 0; j < 4 && i4 + j < n; ++j) out[i4 + j] = z[j];
}
__global__ void counter_bump_kernel(long long* counter) { if (threadIdx.x == 0 && blockIdx.x == 0) *counter += 1; }

extern "C" int spv_counter_bump(int64_t* counter, void* stream) {
  if (!counter) return fail(SPV_ERR_ARG, "spv_counter_bump: null counter%s");
  hipLaunchKernelGGL(counter_bump_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (long long*)counter);
  return launch_status("spv_counter_bump");
}

extern "C" int spv_randn(float* out, int64_t n, const int64_t* counter, uint64_t key, void* stream) {
  if (!out || n < 0) return fail(SPV_ERR_ARG, "spv_randn: bad arguments%s");
  if (n == 0) return SPV_OK;
  hipLaunchKernelGGL(randn_kernel, dim3((unsigned)((n + 1023) / 1024)), dim3(256), 0, (hipStream_t)stream, out, (long)n, (const long long*)counter, (unsigned long long)key);
  return launch_status("spv_randn");
}

// Adam that also refreshes the bf16 operand images of the matrices it has just updated (the fc1 weights of both encoders, the
// mixing head's [W_m | b_m]): the step that follows then starts without its spv_pack_bf16 launches.  Same arithmetic as
// adam_kernel; per 4-element chunk one range test per image (<= SPV_ADAM_MAX_IMAGES, all warp-uniform but at range borders).
struct AdamImages { int n; spv_adam_image img[SPV_ADAM_MAX_IMAGES]; };
// [begin, begin + count) ranges of the flat buffer the launch leaves alone (their parameters were updated where their gradient was
// produced: spv_reduce_slabs_adam), ascending and disjoint, on 4-element boundaries.  The grid walks the n_kept elements that remain
// and maps each 4-chunk to its place in the buffer: a skipped chunk costs neither a loop trip nor memory traffic.
struct AdamSkips { int n; long begin[SPV_ADAM_MAX_SKIP], count[SPV_ADAM_MAX_SKIP]; };

__global__ void adam_images_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                   long n_kept, float lr, float b1, float b2, float eps, float wd, float bc1, float bc2, float gscale, AdamImages im,
                                   AdamSkips sk, long long* step_counter, const long long* t_dev, double b1d, double b2d) {
  if (step_counter && blockIdx.x == 0 && threadIdx.x == 0) *step_counter += 1;   // (read by the NEXT step's spv_randn / dropout: stream order)
  const AdamStep a = adam_prologue(lr, b1, b2, eps, wd, bc1, bc2, gscale, t_dev, b1d, b2d);
  const long stride = (long)gridDim.x * blockDim.x * 4;
  for (long ik = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4; ik < n_kept; ik += stride) {
    float out[4];
    const int cnt = (ik + 4 <= n_kept) ? 4 : (int)(n_kept - ik);
    long i = ik;   // the chunk's offset in the buffer: past every skipped range that begins at or before it
    for (int d = 0; d < sk.n; ++d) i += i >= sk.begin[d] ? sk.count[d] : 0;
    if (cnt == 4) {
      f4v pp = *reinterpret_cast<f4v*>(p + i), gg = *reinterpret_cast<const f4v*>(g + i);
      f4v mm = *reinterpret_cast<f4v*>(m + i), vv = *reinterpret_cast<f4v*>(v + i);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float pj = pp[j], mj = mm[j], vj = vv[j];
        adam_update(pj, gg[j], mj, vj, a);
        pp[j] = pj; mm[j] = mj; vv[j] = vj;
        out[j] = pj;
      }
      *reinterpret_cast<f4v*>(p + i) = pp; *reinterpret_cast<f4v*>(m + i) = mm; *reinterpret_cast<f4v*>(v + i) = vv;
    } else {
      for (int j = 0; j < cnt; ++j) {
        const long k = i + j;
        adam_update(p[k], g[k], m[k], v[k], a);
        out[j] = p[k];
      }
    }
    for (int d = 0; d < im.n; ++d) {
      const spv_adam_image& q = im.img[d];
      const long k0 = i - q.begin;
      if (k0 + cnt <= 0 || k0 >= q.count) continue;
      // (parameters start on 4-element boundaries of the flat buffer, so k0 >= 0 here)
      adam_image_store(q, k0, cnt, out);
      break;   // ranges are disjoint
    }
  }
}

static bool adam_image_ok(const spv_adam_image& q) {   // (everything but the image's place in a flat buffer)
  return q.dst && q.count > 0 && q.cols > 0 && q.ld >= q.cols + q.col_off && q.row_off >= 0 && q.col_off >= 0 && q.count < (1L << 31) &&
         (q.fmt == SPV_IMAGE_BF16 || (q.fmt == SPV_IMAGE_F16 && q.scale > 0.f));
}

extern "C" int spv_adam_step_images(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                                    float weight_decay, float bc1, float bc2, float grad_scale, const spv_adam_image* images, int32_t n_images,
                                    const spv_adam_range* skip, int32_t n_skip, int64_t* step_counter, const int64_t* t_dev, double beta1_d,
                                    double beta2_d, void* stream) {
  if (!p || !g || !m || !v || n < 0 || n_images < 0 || n_images > SPV_ADAM_MAX_IMAGES || (n_images && !images) || n_skip < 0 ||
      n_skip > SPV_ADAM_MAX_SKIP || (n_skip && !skip))
    return fail(SPV_ERR_ARG, "spv_adam_step_images: bad arguments%s");
  if (n == 0) return SPV_OK;
  if ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(v)) & 15)
    return fail(SPV_ERR_ARG, "spv_adam_step_images: buffers must be 16-byte aligned%s");
  AdamImages im{};
  im.n = n_images;
  for (int d = 0; d < n_images; ++d) {
    const spv_adam_image& q = images[d];
    if (!adam_image_ok(q) || q.begin < 0 || (q.begin & 3) || q.begin + q.count > n)
      return fail(SPV_ERR_ARG, "spv_adam_step_images: bad image descriptor%s");
    im.img[d] = q;
  }
  AdamSkips sk{};
  sk.n = n_skip;
  long n_kept = n, end = 0;
  for (int d = 0; d < n_skip; ++d) {   // ascending, disjoint, whole 4-chunks (a range that ends the buffer may end anywhere)
    const spv_adam_range& r = skip[d];
    if (r.begin < end || (r.begin & 3) || r.count <= 0 || r.begin + r.count > n || ((r.count & 3) && r.begin + r.count != n))
      return fail(SPV_ERR_ARG, "spv_adam_step_images: bad skip range%s");
    sk.begin[d] = r.begin; sk.count[d] = r.count;
    end = r.begin + r.count;
    n_kept -= r.count;
  }
  if (n_kept == 0) {   // nothing left to update: the step counter still advances
    return step_counter ? spv_counter_bump(step_counter, stream) : SPV_OK;
  }
  long blocks = (n_kept / 4 + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(adam_images_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n_kept, lr, beta1, beta2, eps,
                     weight_decay, bc1, bc2, grad_scale, im, sk, (long long*)step_counter, (const long long*)t_dev, beta1_d, beta2_d);
  return launch_status("spv_adam_step_images");
}

// slab sums whose parameters take their Adam step in the same launch (reduce_adam_fused_kernel, spv_small.h)
extern "C" int spv_reduce_slabs_adam(const spv_reduce_adam_batch* b, float lr, float beta1, float beta2, float eps, float weight_decay,
                                     float bc1, float bc2, float grad_scale, const int64_t* t_dev, double beta1_d, double beta2_d, void* stream) {
  if (!b || b->nprob <= 0 || b->nprob > SPV_MAXRA) return fail(SPV_ERR_ARG, "spv_reduce_slabs_adam: bad batch%s");
  ReduceAdamArgs a{};
  a.nprob = b->nprob;
  long blocks = 1;
  for (int i = 0; i < b->nprob; ++i) {
    const spv_reduce_adam_prob& q = b->p[i];
    const spv_reduce_prob& r = q.r;
    if (!r.src || !r.dst || r.nslabs <= 0 || r.nslabs > RED_FEW_MAX || r.rows <= 0 || r.cols <= 0 || r.ld_src < r.col_off + r.cols || r.col_off < 0 ||
        (long)r.rows * r.cols >= (1l << 31) || r.ld_dst != r.cols || r.accumulate || r.exp_scale || !q.p || !q.m || !q.v)
      return fail(SPV_ERR_ARG, "spv_reduce_slabs_adam: bad problem%s");
    if (q.img.dst && (!adam_image_ok(q.img) || q.img.cols != r.cols || q.img.count != (long)r.rows * r.cols))
      return fail(SPV_ERR_ARG, "spv_reduce_slabs_adam: bad image descriptor%s");
    a.p[i] = q;
    long t = ((long)r.rows * r.cols + 255) / 256;   // one pass; beyond 8192 workgroups a grid-stride loop
    if (t > 8192) t = 8192;
    a.nblk[i] = (unsigned)t;
    if (t > blocks) blocks = t;
  }
  a.lr = lr; a.b1 = beta1; a.b2 = beta2; a.eps = eps; a.wd = weight_decay; a.bc1 = bc1; a.bc2 = bc2; a.gscale = grad_scale;
  a.t_dev = (const long long*)t_dev; a.b1d = beta1_d; a.b2d = beta2_d;
  hipLaunchKernelGGL(reduce_adam_fused_kernel, dim3((unsigned)blocks, b->nprob), dim3(256), 0, (hipStream_t)stream, a);
  return launch_status("spv_reduce_slabs_adam");
}

extern "C" int spv_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                             float eps, float weight_decay, float bc1, float bc2, float grad_scale, void* stream) {
  if (!p || !g || !m || !v || n < 0) return fail(SPV_ERR_ARG, "spv_adam_step: bad arguments%s");
  if (n == 0) return SPV_OK;
  if ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(v)) & 15)
    return fail(SPV_ERR_ARG, "spv_adam_step: buffers must be 16-byte aligned%s");
  long blocks = (n / 4 + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(adam_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, g, m, v, (long)n, lr, beta1, beta2, eps,
                     weight_decay, bc1, bc2, grad_scale);
  return launch_status("spv_adam_step");
}

// ---------------------------------------------------------------------------------------------
// small dense primitives (spv_small.h)
// ---------------------------------------------------------------------------------------------
static int check_linear(const spv_linear_batch* a, const char* who) {
  if (!a || a->nprob <= 0 || a->nprob > SPV_MAXP || a->B <= 0) return fail(SPV_ERR_ARG, "%s: bad batch", who);
  if (a->drop_p < 0.f || a->drop_p >= 1.f) return fail(SPV_ERR_ARG, "%s: dropout probability outside [0,1)", who);
  for (int i = 0; i < a->nprob; ++i)
    if (a->p[i].N <= 0 || a->p[i].K <= 0 || !a->p[i].W) return fail(SPV_ERR_ARG, "%s: bad problem", who);
  return SPV_OK;
}
static void linear_extents(const spv_linear_batch* a, int& nmax, int& kmax) {
  nmax = kmax = 0;
  for (int i = 0; i < a->nprob; ++i) { nmax = a->p[i].N > nmax ? a->p[i].N : nmax; kmax = a->p[i].K > kmax ? a->p[i].K : kmax; }
}

extern "C" int spv_linear_fwd(const spv_linear_batch* a, void* stream) {
  int rc = check_linear(a, "spv_linear_fwd");
  if (rc) return rc;
  for (int i = 0; i < a->nprob; ++i) if (!a->p[i].X || !a->p[i].Y) return fail(SPV_ERR_ARG, "spv_linear_fwd: null pointer%s");
  int nmax, kmax; linear_extents(a, nmax, kmax);
  int rows = a->B;
  for (int i = 0; i < a->nprob; ++i) {
    const spv_linear_prob& q = a->p[i];
    if (q.img_hi && (q.ld_img < q.N || q.img_rows < 0)) return fail(SPV_ERR_ARG, "spv_linear_fwd: bad operand image%s");
    if (q.img_hi && q.img_rows > rows) rows = q.img_rows;   // the image's padding rows are zero filled by the same launch
  }
  hipLaunchKernelGGL(linear_fwd_kernel, dim3((rows + 63) / 64, (nmax + 63) / 64, a->nprob), dim3(256), 0, (hipStream_t)stream, *a);
  return launch_status("spv_linear_fwd");
}
// the checks of an input-gradient batch (spv_linear_dgrad, the `d` batch of spv_linear_bwd)
static int check_linear_dgrad(const spv_linear_batch* a, const char* who) {
  int rc = check_linear(a, who);
  if (rc) return rc;
  for (int i = 0; i < a->nprob; ++i)
    if (!a->p[i].dY || !a->p[i].dX || ((a->relu || a->drop_p > 0.f) && !a->p[i].Y)) return fail(SPV_ERR_ARG, "%s: null pointer", who);
  return SPV_OK;
}
// ... of a weight-gradient batch (spv_linear_wgrad, the `w` batch of spv_linear_bwd)
static int check_linear_wgrad(const spv_linear_batch* a, const char* who) {
  int rc = check_linear(a, who);
  if (rc) return rc;
  for (int i = 0; i < a->nprob; ++i)
    if (!a->p[i].dY || !a->p[i].X || !a->p[i].dW || ((a->relu || a->drop_p > 0.f) && !a->p[i].Y)) return fail(SPV_ERR_ARG, "%s: null pointer", who);
  return SPV_OK;
}
// ... and of that batch's partial-sum workspace; gives the batch's extents and prob_stride, the workspace elements per problem
static int check_linear_wpart(const spv_linear_batch* a, const float* wpart, int64_t wpart_elems, const char* who, int& nmax, int& kmax, long& prob_stride) {
  if (!wpart) return fail(SPV_ERR_ARG, "%s: workspace missing", who);
  linear_extents(a, nmax, kmax);
  prob_stride = (long)WG_SLICES * nmax * (kmax + 1);
  if (wpart_elems < prob_stride * a->nprob) return fail(SPV_ERR_ARG, "%s: workspace too small", who);
  return SPV_OK;
}

extern "C" int spv_linear_dgrad(const spv_linear_batch* a, void* stream) {
  int rc = check_linear_dgrad(a, "spv_linear_dgrad");
  if (rc) return rc;
  int nmax, kmax; linear_extents(a, nmax, kmax);
  hipLaunchKernelGGL(linear_dgrad_kernel, dim3((a->B + 63) / 64, (kmax + 63) / 64, a->nprob), dim3(256), 0, (hipStream_t)stream, *a);
  return launch_status("spv_linear_dgrad");
}
extern "C" int spv_linear_wgrad(const spv_linear_batch* a, float* wpart, int64_t wpart_elems, void* stream) {
  int nmax, kmax;
  long prob_stride;
  int rc = check_linear_wgrad(a, "spv_linear_wgrad");
  if (rc == SPV_OK) rc = check_linear_wpart(a, wpart, wpart_elems, "spv_linear_wgrad", nmax, kmax, prob_stride);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (a->B <= WG_DIRECT_MAX_B) {   // one slice holds the whole minibatch: results straight into dW / db
    hipLaunchKernelGGL(linear_wgrad_direct_kernel, dim3((nmax + 31) / 32, (kmax + 31) / 32, a->nprob), dim3(256), 0, s, *a);
    return launch_status("spv_linear_wgrad");
  }
  hipLaunchKernelGGL(linear_wgrad_kernel, dim3((nmax + 31) / 32, (kmax + 31) / 32, a->nprob * WG_SLICES), dim3(256), 0, s, *a, wpart, prob_stride);
  hipLaunchKernelGGL(linear_wgrad_reduce_kernel, dim3((unsigned)(((long)nmax * (kmax + 1) + 255) / 256), a->nprob), dim3(256), 0, s, *a, wpart, prob_stride);
  return launch_status("spv_linear_wgrad");
}

// checks a pending-reduce record; rgx = workgroups per problem of its reduction (linear_wgrad_reduce_kernel's grid x)
static int check_pending(const spv_linear_pending* r, const char* who, int& rgx) {
  if (r->nprob <= 0 || r->nprob > SPV_MAXP || !r->wpart) return fail(SPV_ERR_ARG, "%s: bad pending record", who);
  int nmax = 0, kmax = 0;
  for (int i = 0; i < r->nprob; ++i) {
    const spv_linear_pending_prob& t = r->p[i];
    if (t.N <= 0 || t.K <= 0 || !t.dW) return fail(SPV_ERR_ARG, "%s: bad pending problem", who);
    nmax = t.N > nmax ? t.N : nmax; kmax = t.K > kmax ? t.K : kmax;
  }
  if (r->prob_stride < (int64_t)WG_SLICES * nmax * (kmax + 1)) return fail(SPV_ERR_ARG, "%s: pending problem stride too small", who);
  rgx = (int)(((long)nmax * (kmax + 1) + 255) / 256);
  return SPV_OK;
}
extern "C" int spv_linear_reduce_pending(const spv_linear_pending* pending, void* stream) {
  if (!pending) return fail(SPV_ERR_ARG, "spv_linear_reduce_pending: null record%s");
  int rgx = 0;
  int rc = check_pending(pending, "spv_linear_reduce_pending", rgx);
  if (rc) return rc;
  hipLaunchKernelGGL(linear_pending_reduce_kernel, dim3(rgx, pending->nprob), dim3(256), 0, (hipStream_t)stream, *pending);
  return launch_status("spv_linear_reduce_pending");
}
extern "C" int spv_linear_bwd(const spv_linear_batch* d, const spv_linear_batch* w, float* wpart, int64_t wpart_elems,
                              const spv_linear_pending* pending, void* stream) {
  if (!d && !w) {
    if (!pending) return fail(SPV_ERR_ARG, "spv_linear_bwd: nothing to do%s");
    return spv_linear_reduce_pending(pending, stream);
  }
  static const spv_linear_batch none = {};
  LinearBwdGrid g = {};
  long prob_stride = 0;
  if (d) {   // spv_linear_dgrad's checks and grid
    int rc = check_linear_dgrad(d, "spv_linear_bwd");
    if (rc) return rc;
    int nmax, kmax; linear_extents(d, nmax, kmax);
    g.dgx = (d->B + 63) / 64; g.dgy = (kmax + 63) / 64;
    g.nd = g.dgx * g.dgy * d->nprob;
  }
  if (w) {   // spv_linear_wgrad's
    int nmax, kmax;
    int rc = check_linear_wgrad(w, "spv_linear_bwd");
    if (rc) return rc;
    if (w->accumulate) return fail(SPV_ERR_ARG, "spv_linear_bwd: accumulate belongs to the input-gradient batch%s");
    rc = check_linear_wpart(w, wpart, wpart_elems, "spv_linear_bwd", nmax, kmax, prob_stride);
    if (rc) return rc;
    g.wgx = (nmax + 31) / 32; g.wgy = (kmax + 31) / 32;
    g.nw = g.wgx * g.wgy * w->nprob * (w->B <= WG_DIRECT_MAX_B ? 1 : WG_SLICES);
  }
  if (d && w && (d->B != w->B || (d->relu != 0) != (w->relu != 0) || d->drop_p != w->drop_p))
    return fail(SPV_ERR_ARG, "spv_linear_bwd: the two batches disagree in B / relu / drop_p%s");
  int nr = 0;
  if (pending) {
    int rc = check_pending(pending, "spv_linear_bwd", g.rgx);
    if (rc) return rc;
    if (w) {   // this launch's partials must not land in the workspace it sums
      const float* pe = pending->wpart + pending->prob_stride * pending->nprob;
      if (wpart < pe && pending->wpart < wpart + wpart_elems) return fail(SPV_ERR_ARG, "spv_linear_bwd: wpart overlaps the pending workspace%s");
    }
    nr = g.rgx * pending->nprob;
  }
  static const spv_linear_pending no_pending = {};
  hipLaunchKernelGGL(linear_bwd_kernel, dim3((unsigned)(g.nd + g.nw + nr)), dim3(256), 0, (hipStream_t)stream, d ? *d : none, w ? *w : none,
                     pending ? *pending : no_pending, g, wpart, prob_stride);
  return launch_status("spv_linear_bwd");
}

static int check_bn(const spv_bn_batch* a, const char* who) {
  if (!a || a->nprob <= 0 || a->nprob > SPV_MAXP || a->B <= 0) return fail(SPV_ERR_ARG, "%s: bad batch", who);
  for (int i = 0; i < a->nprob; ++i) {
    const spv_bn_prob& q = a->p[i];
    if (q.N <= 0 || q.N > 256 || !q.X || !q.gamma || !q.beta || !q.running_mean || !q.running_var || !q.stats || !q.part)
      return fail(SPV_ERR_ARG, "%s: bad problem (N <= 256, non-null pointers)", who);
  }
  return SPV_OK;
}
static bool bn_all_narrow(const spv_bn_batch* a) {   // every problem N <= 64: the consumers finalise the statistics themselves
  for (int i = 0; i < a->nprob; ++i) if (a->p[i].N > 64) return false;
  return true;
}
extern "C" int spv_bn_fwd(const spv_bn_batch* a, void* stream) {
  int rc = check_bn(a, "spv_bn_fwd");
  if (rc) return rc;
  for (int i = 0; i < a->nprob; ++i) if (!a->p[i].Y) return fail(SPV_ERR_ARG, "spv_bn_fwd: null output%s");
  dim3 grid((a->B + BN_ROWS - 1) / BN_ROWS, a->nprob);
  hipStream_t s = (hipStream_t)stream;
  int nmax = 0;
  for (int i = 0; i < a->nprob; ++i) nmax = a->p[i].N > nmax ? a->p[i].N : nmax;
  if (a->training) hipLaunchKernelGGL(bn_stats_kernel, grid, dim3(256), 0, s, *a);
  int rmax = a->B;
  for (int i = 0; i < a->nprob; ++i) if (a->p[i].img_hi && a->p[i].img_rows > rmax) rmax = a->p[i].img_rows;
  const dim3 agrid((rmax + BN_ROWS - 1) / BN_ROWS, a->nprob);
  if (bn_all_narrow(a)) {   // two launches: every workgroup of the second re-derives its columns' statistics from the partials
    hipLaunchKernelGGL(bn_apply_fin_kernel, agrid, dim3(256), 0, s, *a);
  } else {
    hipLaunchKernelGGL(bn_finalize_kernel, dim3((nmax + 63) / 64, a->nprob), dim3(256), 0, s, *a);
    hipLaunchKernelGGL(bn_apply_kernel, agrid, dim3(256), 0, s, *a);
  }
  return launch_status("spv_bn_fwd");
}
extern "C" int spv_bn_bwd(const spv_bn_batch* a, void* stream) {
  int rc = check_bn(a, "spv_bn_bwd");
  if (rc) return rc;
  for (int i = 0; i < a->nprob; ++i)
    if (!a->p[i].dY || !a->p[i].dX || !a->p[i].dgamma || !a->p[i].dbeta || (a->relu && !a->p[i].Y)) return fail(SPV_ERR_ARG, "spv_bn_bwd: null pointer%s");
  dim3 grid((a->B + BN_ROWS - 1) / BN_ROWS, a->nprob);
  hipStream_t s = (hipStream_t)stream;
  int nmax = 0;
  for (int i = 0; i < a->nprob; ++i) nmax = a->p[i].N > nmax ? a->p[i].N : nmax;
  hipLaunchKernelGGL(bn_bwd_reduce_kernel, grid, dim3(256), 0, s, *a);
  if (bn_all_narrow(a)) {
    hipLaunchKernelGGL(bn_bwd_apply_fin_kernel, grid, dim3(256), 0, s, *a);
  } else {
    hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3((nmax + 63) / 64, a->nprob), dim3(256), 0, s, *a);
    hipLaunchKernelGGL(bn_bwd_apply_kernel, grid, dim3(256), 0, s, *a);
  }
  return launch_status("spv_bn_bwd");
}

static int check_sample(const spv_sample_batch* a, const char* who) {
  if (!a || a->nprob <= 0 || a->nprob > SPV_MAXP || a->B <= 0) return fail(SPV_ERR_ARG, "%s: bad batch", who);
  for (int i = 0; i < a->nprob; ++i)
    if (a->p[i].n <= 0 || a->p[i].n > 32 || !a->p[i].post || !a->p[i].eps || !a->p[i].scale) return fail(SPV_ERR_ARG, "%s: bad problem", who);
  return SPV_OK;
}
// encoder heads in two launches per direction (csrc/spv_small.h: enc_heads_*): bn->p[2e], bn->p[2e + 1] = the BatchNorm problems of
// encoder e's mu / logvar heads, sb->p[e] its sampling problem
static int check_heads(const spv_bn_batch* bn, const spv_sample_batch* sb, const char* who) {
  int rc = check_bn(bn, who);
  if (rc) return rc;
  rc = check_sample(sb, who);
  if (rc) return rc;
  if (bn->nprob != 2 * sb->nprob || bn->B != sb->B || bn->relu) return fail(SPV_ERR_ARG, "%s: two BatchNorm problems per sampling problem, same batch, no relu", who);
  for (int e = 0; e < sb->nprob; ++e) {
    const spv_bn_prob &q0 = bn->p[2 * e], &q1 = bn->p[2 * e + 1];
    const int n = sb->p[e].n;
    if (q0.N != n || q1.N != n || q0.img_hi || q1.img_hi) return fail(SPV_ERR_ARG, "%s: head widths differ from the sampling problem's n", who);
    if (q0.Y != sb->p[e].post || q1.Y != sb->p[e].post + n || q0.ldy != 2 * n || q1.ldy != 2 * n)
      return fail(SPV_ERR_ARG, "%s: the BatchNorm outputs must be the two halves of the sampling problem's post [B][2n]", who);
  }
  return SPV_OK;
}
extern "C" int spv_enc_heads_fwd(const spv_bn_batch* bn, const spv_sample_batch* sb, void* stream) {
  int rc = check_heads(bn, sb, "spv_enc_heads_fwd");
  if (rc) return rc;
  for (int i = 0; i < sb->nprob; ++i) if (!sb->p[i].logz || !sb->p[i].theta || !sb->p[i].kl) return fail(SPV_ERR_ARG, "spv_enc_heads_fwd: null output%s");
  hipStream_t s = (hipStream_t)stream;
  const unsigned nb = (bn->B + BN_ROWS - 1) / BN_ROWS;
  if (bn->training) hipLaunchKernelGGL(bn_stats_kernel, dim3(nb, bn->nprob), dim3(256), 0, s, *bn);
  hipLaunchKernelGGL(enc_heads_bn_sample_fwd_kernel, dim3(nb, sb->nprob), dim3(256), 0, s, *bn, *sb);
  return launch_status("spv_enc_heads_fwd");
}
extern "C" int spv_enc_heads_bwd(const spv_bn_batch* bn, const spv_sample_batch* sb, void* stream) {
  int rc = check_heads(bn, sb, "spv_enc_heads_bwd");
  if (rc) return rc;
  for (int i = 0; i < sb->nprob; ++i) if (!sb->p[i].d_post) return fail(SPV_ERR_ARG, "spv_enc_heads_bwd: null output%s");
  for (int i = 0; i < bn->nprob; ++i) {
    const spv_bn_prob& q = bn->p[i];
    if (!q.dX || !q.dgamma || !q.dbeta) return fail(SPV_ERR_ARG, "spv_enc_heads_bwd: null pointer%s");
    const int e = i / 2, n = sb->p[e].n;
    if (q.dY != sb->p[e].d_post + (i & 1) * n || q.lddy != 2 * n) return fail(SPV_ERR_ARG, "spv_enc_heads_bwd: dY must be the halves of d_post [B][2n]%s");
  }
  if (!bn->training) return fail(SPV_ERR_UNSUPPORTED, "spv_enc_heads_bwd: training-mode BatchNorm only (use spv_enc_sample_bwd + spv_bn_bwd)%s");
  hipStream_t s = (hipStream_t)stream;
  const unsigned nb = (bn->B + BN_ROWS - 1) / BN_ROWS;
  hipLaunchKernelGGL(enc_heads_bwd_reduce_kernel, dim3(nb, sb->nprob), dim3(256), 0, s, *bn, *sb);
  hipLaunchKernelGGL(bn_bwd_apply_fin_kernel, dim3(nb, bn->nprob), dim3(256), 0, s, *bn);
  return launch_status("spv_enc_heads_bwd");
}

extern "C" int spv_enc_sample_fwd(const spv_sample_batch* a, void* stream) {
  int rc = check_sample(a, "spv_enc_sample_fwd");
  if (rc) return rc;
  for (int i = 0; i < a->nprob; ++i) if (!a->p[i].logz || !a->p[i].theta || !a->p[i].kl) return fail(SPV_ERR_ARG, "spv_enc_sample_fwd: null output%s");
  hipLaunchKernelGGL(enc_sample_fwd_kernel, dim3((a->B + 7) / 8, a->nprob), dim3(256), 0, (hipStream_t)stream, *a);
  return launch_status("spv_enc_sample_fwd");
}
extern "C" int spv_enc_sample_bwd(const spv_sample_batch* a, void* stream) {
  int rc = check_sample(a, "spv_enc_sample_bwd");
  if (rc) return rc;
  for (int i = 0; i < a->nprob; ++i) if (!a->p[i].d_post) return fail(SPV_ERR_ARG, "spv_enc_sample_bwd: null output%s");
  hipLaunchKernelGGL(enc_sample_bwd_kernel, dim3((a->B + 7) / 8, a->nprob), dim3(256), 0, (hipStream_t)stream, *a);
  return launch_status("spv_enc_sample_bwd");
}

// ---------------------------------------------------------------------------------------------
// PoE (label) and decoder preparation
// ---------------------------------------------------------------------------------------------
extern "C" int spv_poe_partner(const float* labels0, const float* labels1, int32_t B0, int32_t B1, int32_t* order0, int32_t* order1,
                               int32_t* rank0, int32_t* rank1, int32_t* tables, int32_t* partner0, int32_t* mode0, int32_t* partner1,
                               int32_t* mode1, int32_t* err, void* stream) {
  if (!labels0 || !labels1 || !order0 || !order1 || !rank0 || !rank1 || !tables || !partner0 || !partner1 || !mode0 || !mode1 || !err || B0 <= 0 || B1 <= 0)
    return fail(SPV_ERR_ARG, "spv_poe_partner: bad arguments%s");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(poe_rank_kernel, dim3(2), dim3(512), 0, s, labels0, labels1, B0, B1, order0, order1, rank0, rank1, tables, err);
  const int Bm = B0 > B1 ? B0 : B1;
  hipLaunchKernelGGL(poe_lookup_kernel, dim3((Bm + 255) / 256, 2), dim3(256), 0, s, labels0, labels1, B0, B1, order0, order1, rank0, rank1,
                     tables, partner0, mode0, partner1, mode1);
  return launch_status("spv_poe_partner");
}
extern "C" int spv_poe_rank(const float* labels0, const float* labels1, int32_t B0, int32_t B1, int32_t* order0, int32_t* order1,
                            int32_t* rank0, int32_t* rank1, int32_t* tables, int32_t* err, void* stream) {
  if (!labels0 || !labels1 || !order0 || !order1 || !rank0 || !rank1 || !tables || !err || B0 <= 0 || B1 <= 0) return fail(SPV_ERR_ARG, "spv_poe_rank: bad arguments%s");
  hipLaunchKernelGGL(poe_rank_kernel, dim3(2), dim3(512), 0, (hipStream_t)stream, labels0, labels1, B0, B1, order0, order1, rank0, rank1, tables, err);
  return launch_status("spv_poe_rank");
}
static int check_poe(const spv_poe_args* a, const char* who) {
  if (!a || a->n <= 0 || a->n > 32 || a->B[0] <= 0 || a->B[1] <= 0) return fail(SPV_ERR_ARG, "%s: bad shape (latent dimension <= 32)", who);
  for (int g = 0; g < 2; ++g)
    if (!a->stats[g] || !a->partner[g] || !a->mode[g] || !a->eps[g] || !a->loc[g] || !a->scale[g] || a->ld[g] < 2 * a->n ||
        (a->expert[g] && a->ld_expert[g] < 2 * a->n))
      return fail(SPV_ERR_ARG, "%s: null pointer / bad pitch", who);
  return SPV_OK;
}
extern "C" int spv_poe_fuse_fwd(const spv_poe_args* a, void* stream) {
  int rc = check_poe(a, "spv_poe_fuse_fwd");
  if (rc) return rc;
  for (int g = 0; g < 2; ++g) if (!a->logvar[g] || !a->logz[g] || !a->theta[g] || !a->kl[g]) return fail(SPV_ERR_ARG, "spv_poe_fuse_fwd: null output%s");
  if (a->lab[0] || a->lab[1]) {
    if (!a->lab[0] || !a->lab[1] || !a->order[0] || !a->order[1] || !a->rank[0] || !a->rank[1] || !a->tables || a->expert[0] || a->expert[1])
      return fail(SPV_ERR_ARG, "spv_poe_fuse_fwd: the label lookup needs lab, order, rank of both groups and tables (and no plan experts)%s");
  }
  const int Bm = a->B[0] > a->B[1] ? a->B[0] : a->B[1];
  hipLaunchKernelGGL(poe_fuse_fwd_kernel, dim3((Bm + 7) / 8, 2), dim3(256), 0, (hipStream_t)stream, *a);
  return launch_status("spv_poe_fuse_fwd");
}
// zero fill as an ordinary kernel launch.  (hipMemsetAsync inside a captured graph becomes a memset node; with two processes sharing the
// GPU the two-rank hipGraph test intermittently -- ~1 run in 10 -- showed NaN gradients in exactly the tensors fed by the buffers these
// memsets clear, as if the fill had not happened before the kernel that accumulates into them; a kernel node has not shown it.)
__global__ void zero_fill_kernel(float* p, long n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) p[i] = 0.f;
}
__global__ void fill_i32_kernel(int32_t* p, long n, int32_t v) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) p[i] = v;
}
static int zero_fill(void* p, size_t bytes, hipStream_t s) {
  const long n = (long)(bytes / 4);
  if (n <= 0) return SPV_OK;
  // DIAGNOSTIC switch (tools/graph_dump.py): the round-2 form, a memset NODE in a captured step, to dump that graph's edges
  static const bool memset_nodes = getenv("SPV_MEMSET_NODES") && atoi(getenv("SPV_MEMSET_NODES")) == 1;
  if (memset_nodes) return hipMemsetAsync(p, 0, bytes, s) == hipSuccess ? SPV_OK : SPV_ERR_LAUNCH;
  hipLaunchKernelGGL(zero_fill_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (float*)p, n);
  return hipGetLastError() == hipSuccess ? SPV_OK : SPV_ERR_LAUNCH;
}

extern "C" int spv_poe_fuse_bwd(const spv_poe_args* a, void* stream) {
  int rc = check_poe(a, "spv_poe_fuse_bwd");
  if (rc) return rc;
  for (int g = 0; g < 2; ++g) if (!a->d_stats[g]) return fail(SPV_ERR_ARG, "spv_poe_fuse_bwd: null output%s");
  const int Bm = a->B[0] > a->B[1] ? a->B[0] : a->B[1];
  const size_t bytes0 = (size_t)a->B[0] * a->ld[0] * sizeof(float);
  const bool adjacent = reinterpret_cast<char*>(a->d_stats[0]) + bytes0 == reinterpret_cast<char*>(a->d_stats[1]);  // one buffer: one memset
  for (int g = 0; g < 2; ++g) {  // the kernel accumulates (own expert + partner's): start from zero
    const size_t bytes = (size_t)a->B[g] * a->ld[g] * sizeof(float);
    if (g == 1 && adjacent) {
    } else if (zero_fill(a->d_stats[g], (g == 0 && adjacent) ? bytes0 + (size_t)a->B[1] * a->ld[1] * sizeof(float) : bytes, (hipStream_t)stream) != SPV_OK)
      return fail(SPV_ERR_LAUNCH, "spv_poe_fuse_bwd: fill failed%s");
    if (a->expert[g]) {
      if (!a->d_expert[g]) return fail(SPV_ERR_ARG, "spv_poe_fuse_bwd: d_expert missing%s");
      if (zero_fill(a->d_expert[g], (size_t)a->B[g] * a->ld_expert[g] * sizeof(float), (hipStream_t)stream) != SPV_OK)
        return fail(SPV_ERR_LAUNCH, "spv_poe_fuse_bwd: fill failed%s");
    }
  }
  if (a->lab[0] != nullptr)   // label PoE: one-to-one pairs
    hipLaunchKernelGGL(poe_fuse_bwd_kernel<false>, dim3((Bm + 7) / 8, 2), dim3(256), 0, (hipStream_t)stream, *a);
  else                        // arg-max partners may coincide: per-workgroup sums per partner, one atomic per column and partner
    hipLaunchKernelGGL(poe_fuse_bwd_kernel<true>, dim3((Bm + 31) / 32, 2), dim3(1024), 0, (hipStream_t)stream, *a);
  return launch_status("spv_poe_fuse_bwd");
}

// ---------------------------------------------------------------------------------------------
// N-group cluster-matched PoE (spv_poe_n.h)
// ---------------------------------------------------------------------------------------------
static int check_poe_comp(const spv_poe_comp_args* a, const char* who, bool bwd) {
  if (!a || a->ngroups < 2 || a->ngroups > SPV_POE_MAXG || a->n <= 0 || a->n > 32 || a->ncomp <= 0 || a->ncomp > SPV_POE_COMP_CMAX || !a->part || !a->mean)
    return fail(SPV_ERR_ARG, "%s: bad shape (2..4 groups, latent dimension <= 32, <= 64 components)", who);
  for (int g = 0; g < a->ngroups; ++g) {
    if (a->B[g] <= 0 || !a->stats[g] || a->ld[g] < 2 * a->n || !a->comp[g] || !a->eps[g] || !a->loc[g] || !a->scale[g]) return fail(SPV_ERR_ARG, "%s: null pointer / bad pitch", who);
    if (!bwd && (!a->logvar[g] || !a->logz[g] || !a->theta[g] || !a->kl[g])) return fail(SPV_ERR_ARG, "%s: null output", who);
    if (bwd && (!a->dpn[g] || !a->d_stats[g])) return fail(SPV_ERR_ARG, "%s: null backward buffer", who);
  }
  return SPV_OK;
}
extern "C" int spv_poe_comp_fwd(const spv_poe_comp_args* a, void* stream) {
  int rc = check_poe_comp(a, "spv_poe_comp_fwd", false);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  int Bm = 0;
  for (int g = 0; g < a->ngroups; ++g) Bm = a->B[g] > Bm ? a->B[g] : Bm;
  const int W = 2 * a->n + 1;
  hipLaunchKernelGGL(pn_stats_kernel, dim3(PN_SEG, a->ngroups), dim3(128), 0, s, *a);
  hipLaunchKernelGGL(pn_means_kernel, dim3((a->ncomp * W + 255) / 256, a->ngroups), dim3(256), 0, s, *a);
  hipLaunchKernelGGL(pn_fuse_fwd_kernel, dim3((Bm + 7) / 8, a->ngroups), dim3(256), 0, s, *a);
  return launch_status("spv_poe_comp_fwd");
}
extern "C" int spv_poe_comp_bwd(const spv_poe_comp_args* a, void* stream) {
  int rc = check_poe_comp(a, "spv_poe_comp_bwd", true);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  int Bm = 0;
  for (int g = 0; g < a->ngroups; ++g) Bm = a->B[g] > Bm ? a->B[g] : Bm;
  hipLaunchKernelGGL(pn_cell_bwd_kernel, dim3((Bm + 7) / 8, a->ngroups), dim3(256), 0, s, *a);
  hipLaunchKernelGGL(pn_comp_bwd_kernel, dim3(PN_SEG, a->ngroups), dim3(64), 0, s, *a);
  hipLaunchKernelGGL(pn_apply_bwd_kernel, dim3((Bm + 7) / 8, a->ngroups), dim3(256), 0, s, *a);
  return launch_status("spv_poe_comp_bwd");
}

extern "C" int spv_zsplit_fwd(const spv_zsplit_args* a, void* stream) {
  if (!a || a->B <= 0 || a->n_p <= 0 || a->n_s <= 0 || a->ngroups <= 0 || a->ngroups > 2) return fail(SPV_ERR_ARG, "spv_zsplit_fwd: bad shape%s");
  for (int g = 0; g < a->ngroups; ++g) if (!a->priv[g] || !a->poe[g] || !a->zcat[g]) return fail(SPV_ERR_ARG, "spv_zsplit_fwd: null pointer%s");
  const long tot = (long)a->B * (a->n_p + a->n_s);
  bool pack = false, pack_all = true;
  for (int g = 0; g < a->ngroups; ++g) { pack = pack || a->am_hi[g] || a->aps_hi[g]; pack_all = pack_all && a->am_hi[g] && a->aps_hi[g]; }
  // with both operand images requested for every group ONE kernel writes zcat and the images (zsplit_pack_kernel computes the latents'
  // positions itself); otherwise zcat first, then whatever images were asked for
  if (!pack_all) hipLaunchKernelGGL(zsplit_fwd_kernel, dim3((unsigned)((tot + 255) / 256), a->ngroups), dim3(256), 0, (hipStream_t)stream, *a);
  if (pack) {
    const int kp = a->kslots ? SPV_DEC_KP_WIDE : SPV_DEC_KP, ks = a->kslots ? SPV_DEC_KS_WIDE : SPV_DEC_KS;
    if (a->Bp < a->B || (a->kslots != 0 && a->kslots != 1) || a->n_p + 1 > kp || a->n_s + 1 > ks || a->am_cols < a->n_p + a->n_s + 1 || a->am_cols < 0 ||
        a->ld_am < a->am_col + a->am_cols)
      return fail(SPV_ERR_ARG, "spv_zsplit_fwd: bad operand-image shape%s");
    const long tp = (long)a->Bp * (kp + ks + a->am_cols);
    if (a->kslots) hipLaunchKernelGGL(zsplit_pack_kernel<2>, dim3((unsigned)((tp + 255) / 256), a->ngroups), dim3(256), 0, (hipStream_t)stream, *a);
    else hipLaunchKernelGGL(zsplit_pack_kernel<1>, dim3((unsigned)((tp + 255) / 256), a->ngroups), dim3(256), 0, (hipStream_t)stream, *a);
  }
  return launch_status("spv_zsplit_fwd");
}
extern "C" int spv_zsplit_bwd(const spv_zsplit_args* a, void* stream) {
  if (!a || a->B <= 0 || a->n_p <= 0 || a->n_s <= 0 || a->ngroups <= 0 || a->ngroups > 2) return fail(SPV_ERR_ARG, "spv_zsplit_bwd: bad shape%s");
  for (int g = 0; g < a->ngroups; ++g) if (!a->d_zcat[g] || !a->d_priv[g] || !a->d_poe[g]) return fail(SPV_ERR_ARG, "spv_zsplit_bwd: null pointer%s");
  const long tot = (long)a->B * (a->n_p + a->n_s);
  hipLaunchKernelGGL(zsplit_bwd_kernel, dim3((unsigned)((tot + 255) / 256), a->ngroups), dim3(256), 0, (hipStream_t)stream, *a);
  return launch_status("spv_zsplit_bwd");
}

static int check_fold(const spv_fold_batch* a, const char* who) {
  if (!a || a->nprob <= 0 || a->nprob > SPV_MAXP || a->B <= 0) return fail(SPV_ERR_ARG, "%s: bad batch", who);
  if (a->kslots != 0 && a->kslots != 1) return fail(SPV_ERR_ARG, "%s: kslots must be 0 or 1", who);
  const int kmax = a->kslots ? FOLD_KMAX_WIDE : FOLD_KMAX;
  for (int i = 0; i < a->nprob; ++i) {
    const spv_fold_prob& q = a->p[i];
    if (q.K <= 0 || q.K > kmax || q.G <= 0 || q.Gp < q.G || !q.W || !q.gamma || !q.beta || !q.running_mean || !q.running_var || !q.stat ||
        (a->training && (!q.zsum || !q.zz)))
      return fail(SPV_ERR_ARG, "%s: bad problem (K <= 32, or 64 with kslots = 1; non-null pointers)", who);
  }
  return SPV_OK;
}
extern "C" int spv_bn_fold_fwd(const spv_fold_batch* a, void* stream) {
  int rc = check_fold(a, "spv_bn_fold_fwd");
  if (rc) return rc;
  int gmax = 0;
  for (int i = 0; i < a->nprob; ++i) {
    const spv_fold_prob& q = a->p[i];
    if (!q.img_hi || !q.img_lo || q.slot < q.K + 1 || q.col_off + q.slot > q.ld_img) return fail(SPV_ERR_ARG, "spv_bn_fold_fwd: bad image slot%s");
    if ((q.slot | q.col_off | q.ld_img) % 8 || ((reinterpret_cast<uintptr_t>(q.img_hi) | reinterpret_cast<uintptr_t>(q.img_lo)) & 15))
      return fail(SPV_ERR_ARG, "spv_bn_fold_fwd: slot, col_off, ld_img must be multiples of 8 elements and the images 16-byte aligned%s");
    gmax = q.Gp > gmax ? q.Gp : gmax;
  }
  if (a->kslots) hipLaunchKernelGGL(bn_fold_fwd_kernel<FOLD_KMAX_WIDE>, dim3((gmax + FOLD_FWD_GENES - 1) / FOLD_FWD_GENES, a->nprob), dim3(256), 0, (hipStream_t)stream, *a);
  else hipLaunchKernelGGL(bn_fold_fwd_kernel<FOLD_KMAX>, dim3((gmax + FOLD_FWD_GENES - 1) / FOLD_FWD_GENES, a->nprob), dim3(256), 0, (hipStream_t)stream, *a);
  return launch_status("spv_bn_fold_fwd");
}
extern "C" int spv_bn_fold_bwd(const spv_fold_batch* a, void* stream) {
  int rc = check_fold(a, "spv_bn_fold_bwd");
  if (rc) return rc;
  int gmax = 0;
  for (int i = 0; i < a->nprob; ++i) {
    const spv_fold_prob& q = a->p[i];
    if (!q.dWeff || !q.dW || !q.dgamma || !q.dbeta || q.ld_dw < q.K + 1 || (a->training && (!q.red_part || !q.z || !q.dz)))
      return fail(SPV_ERR_ARG, "spv_bn_fold_bwd: null pointer%s");
    gmax = q.G > gmax ? q.G : gmax;
  }
  hipStream_t s = (hipStream_t)stream;
  if (a->kslots) hipLaunchKernelGGL(bn_fold_bwd_kernel<FOLD_KMAX_WIDE>, dim3((gmax + 255) / 256, a->nprob), dim3(FOLD_BWD_THREADS), 0, s, *a);
  else hipLaunchKernelGGL(bn_fold_bwd_kernel<FOLD_KMAX>, dim3((gmax + 255) / 256, a->nprob), dim3(FOLD_BWD_THREADS), 0, s, *a);
  if (a->training) {   // (the sum over the gene blocks' partials happens inside zstats_bwd_kernel)
    for (int i = 0; i < a->nprob; ++i) {
      const spv_fold_prob& q = a->p[i];
      if (q.out_priv && (!q.out_poe || q.n_p <= 0 || q.n_s <= 0 || q.zcol < 0 || q.zcol + q.K > q.n_p + q.n_s))
        return fail(SPV_ERR_ARG, "spv_bn_fold_bwd: bad latent-slicing outputs%s");
    }
    if (a->kslots) hipLaunchKernelGGL(zstats_bwd_kernel<FOLD_KMAX_WIDE>, dim3((a->B + 63) / 64, a->nprob), dim3(256), 0, s, *a);
    else hipLaunchKernelGGL(zstats_bwd_kernel<FOLD_KMAX>, dim3((a->B + 63) / 64, a->nprob), dim3(256), 0, s, *a);
  }
  return launch_status("spv_bn_fold_bwd");
}

static int check_trunk(const spv_trunk_batch* a, const char* who) {
  if (!a || a->nprob <= 0 || a->nprob > 2 || a->B <= 0) return fail(SPV_ERR_ARG, "%s: bad batch", who);
  for (int i = 0; i < a->nprob; ++i) {
    const spv_trunk_prob& q = a->p[i];
    if (q.N <= 0 || q.N > 256 || q.K <= 0 || q.K > SPV_TRUNK_KMAX) return fail(SPV_ERR_UNSUPPORTED, "%s: N <= 256 and K <= 48", who);
    if (!q.W || !q.gamma || !q.beta || !q.running_mean || !q.running_var || !q.stat) return fail(SPV_ERR_ARG, "%s: null pointer", who);
    if (a->training && (!q.zsum || !q.zz)) return fail(SPV_ERR_ARG, "%s: training mode needs the z statistics", who);
  }
  return SPV_OK;
}
extern "C" int spv_trunk_fold_fwd(const spv_trunk_batch* a, void* stream) {
  int rc = check_trunk(a, "spv_trunk_fold_fwd");
  if (rc) return rc;
  int nmax = 0;
  for (int i = 0; i < a->nprob; ++i) {
    if (!a->p[i].Wf || !a->p[i].cf) return fail(SPV_ERR_ARG, "spv_trunk_fold_fwd: null output%s");
    nmax = a->p[i].N > nmax ? a->p[i].N : nmax;
  }
  hipLaunchKernelGGL(trunk_fold_fwd_kernel, dim3((nmax + TRUNK_FWD_ROWS - 1) / TRUNK_FWD_ROWS, a->nprob), dim3(1024), 0, (hipStream_t)stream, *a);
  return launch_status("spv_trunk_fold_fwd");
}
extern "C" int spv_trunk_fold_bwd(const spv_trunk_batch* a, void* stream) {
  int rc = check_trunk(a, "spv_trunk_fold_bwd");
  if (rc) return rc;
  for (int i = 0; i < a->nprob; ++i) {
    const spv_trunk_prob& q = a->p[i];
    if (!q.dWf || !q.dcf || !q.dW || !q.dgamma || !q.dbeta) return fail(SPV_ERR_ARG, "spv_trunk_fold_bwd: null pointer%s");
    if (a->training && (!q.dred || !q.z || !q.dz || q.ldz < q.K || q.lddz < q.K)) return fail(SPV_ERR_ARG, "spv_trunk_fold_bwd: z-statistics buffers missing%s");
  }
  hipStream_t s = (hipStream_t)stream;
  int nmax = 0;
  for (int i = 0; i < a->nprob; ++i) nmax = a->p[i].N > nmax ? a->p[i].N : nmax;
  const int nblk = (nmax + TRUNK_BWD_ROWS - 1) / TRUNK_BWD_ROWS;
  hipLaunchKernelGGL(trunk_fold_bwd_kernel, dim3(nblk, a->nprob), dim3(1024), 0, s, *a);
  if (a->training) hipLaunchKernelGGL(trunk_zstats_kernel, dim3((a->B + 63) / 64, a->nprob), dim3(256), 0, s, *a, nblk);
  return launch_status("spv_trunk_fold_bwd");
}

extern "C" int spv_reduce_slabs(const spv_reduce_batch* b, void* stream) {
  if (!b || b->nprob <= 0 || b->nprob > SPV_MAXR) return fail(SPV_ERR_ARG, "spv_reduce_slabs: bad batch%s");
  long blocks = 1;
  for (int i = 0; i < b->nprob; ++i) {
    const spv_reduce_prob& q = b->p[i];
    if (!q.src || !q.dst || q.nslabs <= 0 || q.rows <= 0 || q.cols <= 0 || q.ld_src < q.col_off + q.cols || q.ld_dst < q.cols || q.col_off < 0 ||
        (long)q.rows * q.cols >= (1l << 31))
      return fail(SPV_ERR_ARG, "spv_reduce_slabs: bad problem%s");
    const long t = reduce_blocks_needed(q);   // the grid covers the neediest problem in one pass (beyond 8192 workgroups: grid-stride loops)
    if (t > blocks) blocks = t;
  }
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(reduce_slabs_kernel, dim3((unsigned)blocks, b->nprob), dim3(256), 0, (hipStream_t)stream, *b);
  return launch_status("spv_reduce_slabs");
}

extern "C" int spv_loss_assemble(const float* rec0, const float* rec1, const float* w, const float* const* kl, int32_t nkl, int32_t B,
                                 const float* kl_weight, float* loss, float* rec_sum, float* gkl, void* stream) {
  if (!rec0 || !w || !loss || B <= 0 || nkl < 0 || nkl > 4 || (nkl > 0 && !kl)) return fail(SPV_ERR_ARG, "spv_loss_assemble: bad arguments%s");
  const float* k[4] = {nullptr, nullptr, nullptr, nullptr};
  for (int i = 0; i < nkl; ++i) k[i] = kl[i];   // kl is a HOST array of device pointers
  hipLaunchKernelGGL(loss_assemble_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, rec0, rec1, w, k[0], k[1], k[2], k[3], B, kl_weight,
                     loss, rec_sum, gkl);
  return launch_status("spv_loss_assemble");
}

// relu mask + 16-bit packing of the fc1 output gradient and its column sums (the bias gradients), two launches:
//   fc1_bwd_prep_*: one workgroup per 16 rows, one thread per column: column partial sums of dpre = dh1 * (h1 > 0); split mode
//     (img_lo != NULL, "fp32" precision) also writes the bf16 hi / lo images here; f16 mode records the block's max |dpre| instead;
//   fc1_bwd_finish_*: f16 mode: every workgroup reduces the block maxima (fixed order, <= 1024 values) to the step's power-of-two
//     scale (spv_common.h: pow2_scale_for; the largest element lands in [4096, 8192)), writes f16(dpre * scale) for its 16 rows and
//     workgroup 0 leaves {scale, 1 / scale} in scale_ws[0..1] for the weight-gradient kernel; the first ceil(N1 / 64) workgroups
//     (both modes) sum the column partials in block order into the bias gradients.
// No atomics, no grid synchronisation: the scale is a pure function of dpre, so eager and replayed steps agree bit for bit.
struct Fc1PrepArgs { const float* dh1; const float* h1; int B, N1; bf16_t* img_hi; bf16_t* img_lo; long ld_img; float* part; int nblk; float* db; float* db2; int n_first;
                     float* scale_ws; };   // scale_ws: fp32 [2 + nblk] (f16 mode), NULL in split mode

__device__ __forceinline__ float block_max_256(float v, float* s_red) {   // max over the 256 threads of a workgroup, returned to all of them
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
}

__device__ __forceinline__ void fc1_bwd_prep_body(const Fc1PrepArgs& a, const int blk, float* s_red) {
  const int r0 = blk * 16;
  const bool half = a.img_lo == nullptr;
  float amax = 0.f;
  for (int col = threadIdx.x; col < (int)a.ld_img; col += 256) {
    float sum = 0.f;
#pragma unroll 4
    for (int r = r0; r < r0 + 16; ++r) {
      // (unconditional loads from a clamped address, then a select: a load behind the bounds test is waited for inside that branch)
      const long i = (long)min(r, a.B - 1) * a.N1 + min(col, a.N1 - 1);
      const float hv = a.h1[i], gv = a.dh1[i];
      const float v = (r < a.B && col < a.N1 && hv > 0.f) ? gv : 0.f;
      if (!half) {
        bf16_t hi, lo;
        split_bf16(v, hi, lo);
        a.img_hi[(long)r * a.ld_img + col] = hi;
        a.img_lo[(long)r * a.ld_img + col] = lo;
      }
      amax = fmaxf(amax, fabsf(v));
      sum += v;
    }
    if (col < a.N1) a.part[(long)blk * a.N1 + col] = sum;
  }
  if (half) {
    amax = block_max_256(amax, s_red);
    if (threadIdx.x == 0) a.scale_ws[2 + blk] = amax;
  }
}

__device__ __forceinline__ void fc1_bwd_finish_body(const Fc1PrepArgs& a, const int blk, float* s_red, float (*s_p)[64]) {
  const bool half = a.img_lo == nullptr;
  if (half && blk < a.nblk) {
    float m = 0.f;
    for (int k = threadIdx.x; k < a.nblk; k += 256) m = fmaxf(m, a.scale_ws[2 + k]);
    m = block_max_256(m, s_red);
    float scale, inv;
    pow2_scale_for(m, scale, inv);
    if (blk == 0 && threadIdx.x == 0) { a.scale_ws[0] = scale; a.scale_ws[1] = inv; }
    const int r0 = blk * 16;
    for (int col = threadIdx.x; col < (int)a.ld_img; col += 256) {
#pragma unroll 4
      for (int r = r0; r < r0 + 16; ++r) {
        const long i = (long)min(r, a.B - 1) * a.N1 + min(col, a.N1 - 1);
        const float hv = a.h1[i], gv = a.dh1[i];
        const float v = (r < a.B && col < a.N1 && hv > 0.f) ? gv : 0.f;
        a.img_hi[(long)r * a.ld_img + col] = f2h(v * scale);
      }
    }
  }
  if (blk >= (a.N1 + 63) / 64) return;   // (workgroup-uniform)
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int col = blk * 64 + tx;
  float v = 0.f;
  if (col < a.N1)
#pragma unroll 8
    for (int k = ty; k < a.nblk; k += 4) v += a.part[(long)k * a.N1 + col];
  s_p[ty][tx] = v;
  __syncthreads();
  if (ty != 0 || col >= a.N1) return;
  v = ((s_p[0][tx] + s_p[1][tx]) + s_p[2][tx]) + s_p[3][tx];
  if (a.db2 != nullptr && col >= a.n_first) a.db2[col - a.n_first] = v;
  else a.db[col] = v;
}

__global__ __launch_bounds__(256) void fc1_bwd_prep_kernel(Fc1PrepArgs a) {
  __shared__ float s_red[4];
  fc1_bwd_prep_body(a, blockIdx.x, s_red);
}
__global__ __launch_bounds__(256) void fc1_bwd_finish_kernel(Fc1PrepArgs a) {
  __shared__ float s_red[4];
  __shared__ float s_p[4][64];
  fc1_bwd_finish_body(a, blockIdx.x, s_red, s_p);
}
__global__ __launch_bounds__(256) void fc1_bwd_prep_pair_kernel(Fc1PrepArgs a0, Fc1PrepArgs a1) {   // blockIdx.y = group
  __shared__ float s_red[4];
  const Fc1PrepArgs a = blockIdx.y ? a1 : a0;
  if ((int)blockIdx.x >= a.nblk) return;
  fc1_bwd_prep_body(a, blockIdx.x, s_red);
}
__global__ __launch_bounds__(256) void fc1_bwd_finish_pair_kernel(Fc1PrepArgs a0, Fc1PrepArgs a1) {   // blockIdx.y = group
  __shared__ float s_red[4];
  __shared__ float s_p[4][64];
  const Fc1PrepArgs a = blockIdx.y ? a1 : a0;
  fc1_bwd_finish_body(a, blockIdx.x, s_red, s_p);
}
static int fc1_finish_blocks(const Fc1PrepArgs& a) {
  const int nb_bias = (a.N1 + 63) / 64;
  return (a.img_lo == nullptr && a.nblk > nb_bias) ? a.nblk : nb_bias;
}
// (the arguments of spv_enc_fc1_bwd_prep)
static Fc1PrepArgs fc1_prep_args(const float* dh1, const float* h1, int B, int N1, uint16_t* img_hi, uint16_t* img_lo, long ld_img, int Bp, float* part, float* db,
                                 float* db2, int n_first, float* scale_ws) {
  return Fc1PrepArgs{dh1, h1, B, N1, (bf16_t*)img_hi, (bf16_t*)img_lo, ld_img, part, Bp / 16, db, db2, n_first, scale_ws};
}
// the pair forms of spv_enc_fc1_bwd_grouped: 16-bit mode only, so the f16 image (no lo plane) whatever dh_lo says
static Fc1PrepArgs fc1_prep_args(const spv_fc1_bwd_args& a) {
  return fc1_prep_args(a.dh1, a.h1, a.B, a.N1, a.dh_hi, nullptr, a.ld_dh, a.Bp, a.part, a.db, a.db2, a.n_first, a.scale_ws);
}
// relu mask, image and bias gradients of both groups: one grid per kernel
static void fc1_prep_pair_launch(const spv_fc1_bwd_args& a, const spv_fc1_bwd_args& b, hipStream_t s) {
  const Fc1PrepArgs q0 = fc1_prep_args(a), q1 = fc1_prep_args(b);
  hipLaunchKernelGGL(fc1_bwd_prep_pair_kernel, dim3(max2(q0.nblk, q1.nblk), 2), dim3(256), 0, s, q0, q1);
  hipLaunchKernelGGL(fc1_bwd_finish_pair_kernel, dim3(max2(fc1_finish_blocks(q0), fc1_finish_blocks(q1)), 2), dim3(256), 0, s, q0, q1);
}

extern "C" int spv_enc_fc1_bwd_prep(const float* dh1, const float* h1, int32_t B, int32_t N1, uint16_t* img_hi, uint16_t* img_lo,
                                    int64_t ld_img, int32_t Bp, float* part, float* db, float* db2, int32_t n_first, float* scale_ws, void* stream) {
  if (!dh1 || !h1 || !img_hi || !part || !db) return fail(SPV_ERR_ARG, "spv_enc_fc1_bwd_prep: null pointer%s");
  if (B <= 0 || N1 <= 0 || Bp < B || (Bp % 64) || ld_img < N1) return fail(SPV_ERR_ARG, "spv_enc_fc1_bwd_prep: bad shape (Bp a multiple of 64)%s");
  if (!img_lo && !scale_ws) return fail(SPV_ERR_ARG, "spv_enc_fc1_bwd_prep: the f16 image (img_lo == NULL) needs scale_ws [2 + Bp / 16]%s");
  if (Bp / 16 > 65536) return fail(SPV_ERR_ARG, "spv_enc_fc1_bwd_prep: minibatch too large%s");
  hipStream_t s = (hipStream_t)stream;
  const Fc1PrepArgs a = fc1_prep_args(dh1, h1, B, N1, img_hi, img_lo, ld_img, Bp, part, db, db2, n_first, scale_ws);
  hipLaunchKernelGGL(fc1_bwd_prep_kernel, dim3(a.nblk), dim3(256), 0, s, a);
  hipLaunchKernelGGL(fc1_bwd_finish_kernel, dim3(fc1_finish_blocks(a)), dim3(256), 0, s, a);
  return launch_status("spv_enc_fc1_bwd_prep");
}

// ---- both groups of a step in one launch per kernel (csrc/spv_fc1.h: *_pair_kernel) ---------------------------------------------------
static bool fc1_fwd_dma_ok(const spv_fc1_fwd_args& a) {
  return a.x && a.x->X && a.W1_hi && a.bias && a.slabs && a.h1 && a.library && a.xb_all && a.library_all && a.B > 0 && a.G > 0 && a.splits > 0 &&
         spv_enc_fc1_fwd_uses_dma(a.B, a.G, a.N1, a.nsplit, 1, a.ldw, a.ld_xb) && aligned16(a.xb_all, a.W1_hi) &&
         (a.nsplit == 1 || (a.W1_lo && aligned16(a.W1_lo)));
}
static GemmParams fc1_fwd_dma_params(const spv_fc1_fwd_args& a) {
  GemmParams p{};
  p.A = a.xb_all; p.lda = a.ld_xb; p.B = a.W1_hi; p.ldb = a.ldw; p.rows = a.x->rows;
  if (a.nsplit == 3) p.B_lo = a.W1_lo;   // "fp32" mode: hi / lo planes interleaved inside the image rows, hi / lo weight images
  p.n_cells = a.B; p.n_genes = a.G; p.C = a.slabs; p.ldc = a.N1; p.M = a.B; p.N = a.N1; p.K = a.G;
  const int kt = (a.G + F1_BK - 1) / F1_BK;
  p.k_per_split = ((kt + a.splits - 1) / a.splits) * F1_BK;
  p.c_split_row = a.splits;
  return p;
}

// shapes the LDS-DMA kernel does not take, 16-bit mode on resident images, at most 128 output units (n_hidden <= 64): the register-staged
// GEMM and its epilogue for both groups in one grid each (gemm_pair_kernel) -- at 128 cells per minibatch a launch is mostly fixed cost
static bool fc1_fwd_plain_ok(const spv_fc1_fwd_args& a) {
  return a.x && a.x->X && a.W1_hi && a.bias && a.slabs && a.rowsum_ws && a.h1 && a.library && a.xb_all && a.library_all && a.B > 0 && a.G > 0 && a.splits > 0 &&
         a.nsplit == 1 && a.N1 > 32 && a.N1 <= 128 && (a.ldw % 32) == 0 && a.ldw >= ((a.G + 31) & ~31) && a.ld_xb >= ((a.G + 31) & ~31) && (a.ld_xb % 8) == 0 &&
         (a.cov == nullptr) == (a.cov_idx == nullptr);
}

extern "C" int spv_enc_fc1_fwd_grouped(const spv_fc1_fwd_args* g, int32_t n_groups, void* stream) {
  if (!g || n_groups <= 0) return fail(SPV_ERR_ARG, "spv_enc_fc1_fwd_grouped: bad arguments%s");
  hipStream_t s = (hipStream_t)stream;
  return pairs_then_rest(n_groups,
    [&](int i) {   // the LDS-DMA kernel
      const spv_fc1_fwd_args &a = g[i], &b = g[i + 1];
      if (!(fc1_fwd_dma_ok(a) && fc1_fwd_dma_ok(b) && a.N1 == b.N1 && a.nsplit == b.nsplit)) return NOT_A_PAIR;
      const GemmParams p0 = fc1_fwd_dma_params(a), p1 = fc1_fwd_dma_params(b);
      const int mt0 = (a.B + F1_BM - 1) / F1_BM, mt1 = (b.B + F1_BM - 1) / F1_BM;
      const dim3 grid(mt0 * a.splits + mt1 * b.splits, a.N1 / F1_BN);
      if (a.nsplit == 3) launch_lds<fc1_fwd_dma_split_pair_kernel>(grid, dim3(512), F1_LDS_BYTES, s, p0, p1, mt0 * a.splits);
      else launch_lds<fc1_fwd_dma_pair_kernel>(grid, dim3(512), F1_LDS_BYTES, s, p0, p1, mt0 * a.splits);
      if (int rc = launch_status("spv_enc_fc1_fwd_grouped gemm")) return rc;
      const float acc_scale = (a.nsplit == 1) ? 1.0f / SPV_FC1_W_SCALE : 1.0f;
      const long se0 = (long)mt0 * F1_BM * a.N1, se1 = (long)mt1 * F1_BM * b.N1;
      const Fc1EpiArgs e0{a.slabs, a.splits, se0, a.B, a.N1, a.bias, a.bias2, a.n_first, a.h1, a.library, a.library_all, a.x->rows, acc_scale, a.cov, a.cov_idx};
      const Fc1EpiArgs e1{b.slabs, b.splits, se1, b.B, b.N1, b.bias, b.bias2, b.n_first, b.h1, b.library, b.library_all, b.x->rows, acc_scale, b.cov, b.cov_idx};
      const long sem = se0 > se1 ? se0 : se1;
      hipLaunchKernelGGL(fc1_epilogue_tiled_pair_kernel, dim3((unsigned)((sem / 4 + 255) / 256), 2), dim3(256), 0, s, e0, e1);
      return launch_status("spv_enc_fc1_fwd_grouped epilogue");
    },
    [&](int i) {   // the register-staged kernel
      const spv_fc1_fwd_args &a = g[i], &b = g[i + 1];
      if (!(fc1_fwd_plain_ok(a) && fc1_fwd_plain_ok(b) && a.N1 == b.N1 && a.splits == b.splits)) return NOT_A_PAIR;
      typedef GemmCfg<64, 128, 2, 2, false, false, SRC_GATHER, SRC_PLAIN, unsigned short, 1, 32, 4, 1, true> PlainCfg;
      if (launch_gemm_pair<PlainCfg>(fc1_fwd_params(a, 32), fc1_fwd_params(b, 32), a.splits, s) != SPV_OK) return launch_status("spv_enc_fc1_fwd_grouped gemm pair");
      const float sc = 1.0f / SPV_FC1_W_SCALE;
      const Fc1EpiPlainArgs e0{a.slabs, a.rowsum_ws, a.splits, a.B, a.N1, a.bias, a.bias2, a.n_first, a.h1, a.library, a.library_all, a.x->rows, sc, a.cov, a.cov_idx};
      const Fc1EpiPlainArgs e1{b.slabs, b.rowsum_ws, b.splits, b.B, b.N1, b.bias, b.bias2, b.n_first, b.h1, b.library, b.library_all, b.x->rows, sc, b.cov, b.cov_idx};
      const long tmax = (long)max2(a.B, b.B) * a.N1;
      hipLaunchKernelGGL(fc1_epilogue_pair_kernel, dim3((unsigned)((tmax + 255) / 256), 2), dim3(256), 0, s, e0, e1);
      return launch_status("spv_enc_fc1_fwd_grouped epilogue pair");
    },
    [&](int i) {   // a leftover group, or shapes no pair form takes: the per-group entry point
      const spv_fc1_fwd_args& a = g[i];
      return spv_enc_fc1_fwd(a.x, a.B, a.G, a.W1_hi, a.W1_lo, a.ldw, a.N1, a.bias, a.bias2, a.n_first, a.nsplit, a.splits, a.slabs, a.rowsum_ws, a.h1,
                             a.library, a.xb_all, a.ld_xb, a.library_all, a.cov, a.cov_idx, stream);
    });
}

static bool fc1_bwd_dma_ok(const spv_fc1_bwd_args& a) {
  if (!a.x || !a.x->X || !a.dh1 || !a.h1 || !a.dh_hi || !a.part || !a.db || !a.dW || !a.dW2 || !a.xb || !a.scale_ws || a.B <= 0 || a.G <= 0) return false;
  const int Kpad = (a.B + FW_BK - 1) / FW_BK * FW_BK;
  return a.nsplit == 1 && (a.N1 == FW_BM || a.N1 == 2 * FW_BM) && a.ld_dh == a.N1 && a.n_first == a.N1 / 2 && a.Bp >= Kpad && (a.Bp % 64) == 0 && a.ldc >= a.G &&
         a.ld_xb >= ((a.G + 63) & ~63) && (a.ld_xb % 8) == 0 && fw_lds_bytes(96, Kpad) <= 160 * 1024 && aligned16(a.xb, a.dh_hi);
}

// shapes the LDS-DMA kernel does not take (n_hidden <= 64), 16-bit mode on resident images: prep / finish and the register-staged weight-gradient
// GEMM for both groups in one grid each
static bool fc1_bwd_plain_ok(const spv_fc1_bwd_args& a) {
  return a.x && a.x->X && a.dh1 && a.h1 && a.dh_hi && a.part && a.db && a.dW && a.xb && a.scale_ws && a.B > 0 && a.G > 0 && a.nsplit == 1 &&
         a.N1 > 32 && a.N1 <= 128 && a.Bp >= a.B && (a.Bp % 64) == 0 && a.Bp / 16 <= 65536 && a.ld_dh >= ((a.N1 + 127) & ~127) && (a.ld_dh % 8) == 0 &&
         a.ldc >= a.G && a.ld_xb >= ((a.G + 63) & ~63) && (a.ld_xb % 8) == 0;
}

extern "C" int spv_enc_fc1_bwd_grouped(const spv_fc1_bwd_args* g, int32_t n_groups, void* stream) {
  if (!g || n_groups <= 0) return fail(SPV_ERR_ARG, "spv_enc_fc1_bwd_grouped: bad arguments%s");
  hipStream_t s = (hipStream_t)stream;
  return pairs_then_rest(n_groups,
    [&](int i) {   // the LDS-DMA kernels
      const spv_fc1_bwd_args &a = g[i], &b = g[i + 1];
      if (!(fc1_bwd_dma_ok(a) && fc1_bwd_dma_ok(b) && a.N1 == b.N1)) return NOT_A_PAIR;
      fc1_prep_pair_launch(a, b, s);
      if (int rc = launch_status("spv_enc_fc1_bwd_grouped prep")) return rc;
      GemmParams p[2];
      for (int k = 0; k < 2; ++k) {
        const spv_fc1_bwd_args& c = k ? b : a;
        GemmParams& w = p[k];
        w = GemmParams{};
        w.A = c.dh_hi; w.lda = c.ld_dh; w.B = c.xb; w.ldb = c.ld_xb; w.rows = c.x->rows; w.n_cells = c.B; w.n_genes = c.G;
        w.C = c.dW; w.ldc = c.ldc; w.C2 = c.dW2; w.c_split_row = c.n_first; w.M = c.N1; w.N = c.G; w.K = c.B;
        w.out_scale = c.scale_ws + 1;
      }
      // tile: the one that gets BOTH groups into the fewest rounds of 256 one-per-CU workgroups (64-gene tiles are the faster ones alone)
      const int n64 = (a.G + 63) / 64 + (b.G + 63) / 64, n96 = (a.G + 95) / 96 + (b.G + 95) / 96;
      const int mth = a.N1 / FW_BM;   // 256-unit halves of the dh image (H = 256: one per encoder)
      const bool use96 = (n96 * mth + 255) / 256 < (n64 * mth + 255) / 256;
      const int Kp = max2((a.B + FW_BK - 1) / FW_BK * FW_BK, (b.B + FW_BK - 1) / FW_BK * FW_BK);
      // ... unless a WIDE tile (192 / 256 genes, fc1_wgrad_dma_wide_body) needs fewer ROUNDS of workgroups: a workgroup re-reads the dh image
      // (512 B per cell) beside its 2 t bytes per cell of image rows, so a wide tile is the slower one per workgroup and the faster one only
      // where the narrow tiles need a second round (rocprofv3, us per pair launch: C2 96: 77, 128: 83, 192: 112, 256: 114; G 20 000 96: 154,
      // 192: 123, 256: 125)
      const char* const force_env = getenv("SPV_FC1_WGRAD_TILE");   // (tuning / test switch, read per call: 64 / 96 / 128 / 192 / 256)
      const int force_tile = force_env ? atoi(force_env) : 0;
      int t = use96 ? 96 : 64;
      auto model_us = [&](int tile) {   // every workgroup pulls its bytes at the ONE CU's fill rate, ~32 GB/s measured on every LDS-DMA kernel here, round after round
        const long nwg = (long)((a.G + tile - 1) / tile + (b.G + tile - 1) / tile) * mth;
        return (double)((nwg + 255) / 256) * (double)Kp * (512 + 2 * tile) / 32e3;
      };
      if (Kp >= 512) {
        if (fww_lds_bytes(192, Kp) <= 160 * 1024 && model_us(192) < model_us(t)) t = 192;
        if (fww_lds_bytes(256, Kp) <= 160 * 1024 && model_us(256) < model_us(t)) t = 256;
      }
      if (force_tile == 64 || force_tile == 96 || force_tile == 128 || force_tile == 192 || force_tile == 256) {
        const int need = force_tile >= 192 ? fww_lds_bytes(force_tile, Kp) : fw_lds_bytes(force_tile, Kp);
        if (need <= 160 * 1024) t = force_tile;
      }
      const int lds = t >= 192 ? fww_lds_bytes(t, Kp) : fw_lds_bytes(t, Kp);
      void (*kfn)(GemmParams, GemmParams, int) = t == 256 ? fc1_wgrad_dma_wide_pair_kernel<256> : t == 192 ? fc1_wgrad_dma_wide_pair_kernel<192> :
                                                 t == 96 ? fc1_wgrad_dma_pair_kernel<96> : (t == 128 ? fc1_wgrad_dma_pair_kernel<128> : fc1_wgrad_dma_pair_kernel<64>);
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
      const int nA = (a.G + t - 1) / t, nB = (b.G + t - 1) / t;
      hipLaunchKernelGGL(kfn, dim3(nA + nB, mth), dim3(512), lds, s, p[0], p[1], nA);
      return launch_status("spv_enc_fc1_bwd_grouped wgrad");
    },
    [&](int i) {   // the register-staged kernel
      const spv_fc1_bwd_args &a = g[i], &b = g[i + 1];
      const bool t96a = a.ld_xb >= (a.G + 95) / 96 * 96, t96b = b.ld_xb >= (b.G + 95) / 96 * 96;
      if (!(fc1_bwd_plain_ok(a) && fc1_bwd_plain_ok(b) && a.N1 == b.N1 && t96a == t96b)) return NOT_A_PAIR;
      fc1_prep_pair_launch(a, b, s);
      if (int rc = launch_status("spv_enc_fc1_bwd_grouped prep pair")) return rc;
      const GemmParams p0 = fc1_wgrad_params(a.x, a.B, a.G, a.dh_hi, nullptr, a.ld_dh, a.N1, 1, a.dW, a.dW2, a.n_first, a.ldc, a.xb, a.ld_xb, a.scale_ws);
      const GemmParams p1 = fc1_wgrad_params(b.x, b.B, b.G, b.dh_hi, nullptr, b.ld_dh, b.N1, 1, b.dW, b.dW2, b.n_first, b.ldc, b.xb, b.ld_xb, b.scale_ws);
      int rcg;
      if (t96a) rcg = launch_gemm_pair<GemmCfg<128, 96, 4, 1, true, true, SRC_PLAIN, SRC_GATHER, unsigned short, 1, 64, 4, 1, true>>(p0, p1, 1, s);
      else rcg = launch_gemm_pair<GemmCfg<128, 64, 4, 1, true, true, SRC_PLAIN, SRC_GATHER, unsigned short, 1, 64, 4, 1, true>>(p0, p1, 1, s);
      return rcg != SPV_OK ? launch_status("spv_enc_fc1_bwd_grouped wgrad pair") : SPV_OK;
    },
    [&](int i) {
      const spv_fc1_bwd_args& a = g[i];
      const int rc = spv_enc_fc1_bwd_prep(a.dh1, a.h1, a.B, a.N1, a.dh_hi, a.dh_lo, a.ld_dh, a.Bp, a.part, a.db, a.db2, a.n_first, a.scale_ws, stream);
      if (rc != SPV_OK) return rc;
      return spv_enc_fc1_wgrad(a.x, a.B, a.G, a.dh_hi, a.dh_lo, a.ld_dh, a.N1, a.nsplit, a.dW, a.dW2, a.n_first, a.ldc, a.xb, a.ld_xb, a.scale_ws, stream);
    });
}

extern "C" int spv_plan_invmap(const int32_t* idx0, int32_t B0, const int32_t* idx1, int32_t B1, int32_t* inv0, int32_t n0, int32_t* inv1,
                               int32_t n1, void* stream) {
  if (!idx0 || !idx1 || !inv0 || !inv1 || B0 <= 0 || B1 <= 0 || n0 <= 0 || n1 <= 0) return fail(SPV_ERR_ARG, "spv_plan_invmap: bad arguments%s");
  hipStream_t s = (hipStream_t)stream;
  // (fill kernels, not hipMemsetAsync: see zero_fill)
  hipLaunchKernelGGL(fill_i32_kernel, dim3((unsigned)((n0 + 255) / 256)), dim3(256), 0, s, inv0, (long)n0, -1);
  hipLaunchKernelGGL(fill_i32_kernel, dim3((unsigned)((n1 + 255) / 256)), dim3(256), 0, s, inv1, (long)n1, -1);
  if (hipGetLastError() != hipSuccess) return fail(SPV_ERR_LAUNCH, "spv_plan_invmap: fill failed%s");
  const int Bm = B0 > B1 ? B0 : B1;
  hipLaunchKernelGGL(plan_invmap_kernel, dim3((Bm + 255) / 256, 2), dim3(256), 0, s, idx0, B0, idx1, B1, inv0, n0, inv1, n1);
  return launch_status("spv_plan_invmap");
}

static int check_plan(const spv_plan* p, const char* who) {
  if (!p || !p->ptr0 || !p->ind0 || !p->val0 || !p->ptr1 || !p->ind1 || !p->val1 || p->n0 <= 0 || p->n1 <= 0) return fail(SPV_ERR_ARG, "%s: incomplete plan", who);
  return SPV_OK;
}

extern "C" int spv_plan_argmax(const spv_plan* plan, const int32_t* idx0, const int32_t* idx1, const int32_t* inv0, const int32_t* inv1,
                               int32_t B0, int32_t B1, int32_t* partner0, int32_t* partner1, void* stream) {
  int rc = check_plan(plan, "spv_plan_argmax");
  if (rc) return rc;
  if (!idx0 || !idx1 || !inv0 || !inv1 || !partner0 || !partner1 || B0 <= 0 || B1 <= 0) return fail(SPV_ERR_ARG, "spv_plan_argmax: bad arguments%s");
  const int Bm = B0 > B1 ? B0 : B1;
  hipLaunchKernelGGL(plan_argmax_kernel, dim3((Bm + 255) / 256, 2), dim3(256), 0, (hipStream_t)stream, plan->ptr0, plan->ind0, plan->val0,
                     plan->ptr1, plan->ind1, plan->val1, idx0, idx1, inv0, inv1, B0, B1, plan->n0, plan->n1, partner0, partner1);
  return launch_status("spv_plan_argmax");
}

static int check_expert(const spv_plan_expert_args* a, const char* who) {
  if (!a) return fail(SPV_ERR_ARG, "%s: null arguments", who);
  int rc = check_plan(&a->plan, who);
  if (rc) return rc;
  if (a->B <= 0 || a->n <= 0 || a->n > 32) return fail(SPV_ERR_ARG, "%s: bad shape (latent dimension <= 32)", who);
  for (int g = 0; g < 2; ++g)
    if (!a->idx[g] || !a->inv[g] || !a->comp[g] || !a->stats[g] || !a->rowsum[g] || a->ld[g] < 2 * a->n || a->ld_expert[g] < 2 * a->n)
      return fail(SPV_ERR_ARG, "%s: null pointer / bad pitch", who);
  return SPV_OK;
}
extern "C" int spv_plan_expert_fwd(const spv_plan_expert_args* a, void* stream) {
  int rc = check_expert(a, "spv_plan_expert_fwd");
  if (rc) return rc;
  for (int g = 0; g < 2; ++g) if (!a->expert[g]) return fail(SPV_ERR_ARG, "spv_plan_expert_fwd: null output%s");
  hipLaunchKernelGGL(plan_expert_fwd_kernel, dim3((a->B + 7) / 8, 2), dim3(256), 0, (hipStream_t)stream, *a);
  return launch_status("spv_plan_expert_fwd");
}
extern "C" int spv_plan_expert_bwd(const spv_plan_expert_args* a, void* stream) {
  int rc = check_expert(a, "spv_plan_expert_bwd");
  if (rc) return rc;
  for (int g = 0; g < 2; ++g) if (!a->d_expert[g] || !a->d_stats[g]) return fail(SPV_ERR_ARG, "spv_plan_expert_bwd: null pointer%s");
  hipLaunchKernelGGL(plan_expert_bwd_kernel, dim3((a->B + 7) / 8, 2), dim3(256), 0, (hipStream_t)stream, *a);
  return launch_status("spv_plan_expert_bwd");
}

// f16(log1p(x)) of a whole resident count matrix and library = log(sum_g log1p(x)) per cell, once per data set:
// one workgroup per cell, fixed-order block reduction.
__global__ __launch_bounds__(256) void prepare_log1p_kernel(const void* X, long ldx, int col_off, int is_u16, int G, bf16_t* xb, long ld_xb,
                                                            float* library) {
  __shared__ float s_sum[256];
  const long cell = blockIdx.x;
  float acc = 0.f;
  for (int g = threadIdx.x; g < (int)ld_xb; g += 256) {
    float v = 0.f;
    if (g < G) {
      const float c = is_u16 ? (float)reinterpret_cast<const unsigned short*>(X)[cell * ldx + col_off + g]
                             : reinterpret_cast<const float*>(X)[cell * ldx + col_off + g];
      v = log1p_count(c);
    }
    xb[cell * ld_xb + g] = f2h(v);   // IEEE half: log1p(count) <= 11.1, 11 significant bits (spv_common.h)
    acc += v;
  }
  s_sum[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) s_sum[threadIdx.x] += s_sum[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) library[cell] = __logf(s_sum[0]);
}

// "fp32" mode: bf16 hi / lo planes of log1p(x) interleaved in blocks of 32 genes ([32 hi words | 32 lo words] = 128 bytes per block:
// what one K tile of the LDS-DMA fc1 kernels takes from a row), ld_xb = 2 ldh words per row, + the library
__global__ __launch_bounds__(256) void prepare_log1p_split_kernel(const void* X, long ldx, int col_off, int is_u16, int G, bf16_t* xb, long ld_xb,
                                                                  float* library) {
  __shared__ float s_sum[256];
  const long cell = blockIdx.x;
  const long ldh = ld_xb / 2;
  float acc = 0.f;
  for (int g = threadIdx.x; g < (int)ldh; g += 256) {
    float v = 0.f;
    if (g < G) {
      const float c = is_u16 ? (float)reinterpret_cast<const unsigned short*>(X)[cell * ldx + col_off + g]
                             : reinterpret_cast<const float*>(X)[cell * ldx + col_off + g];
      v = log1p_count(c);
    }
    const bf16_t hi = f2bf(v);
    const long o = cell * ld_xb + (long)(g >> 5) * 64 + (g & 31);
    xb[o] = hi;
    xb[o + 32] = f2bf(v - bf2f(hi));
    acc += v;
  }
  s_sum[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) s_sum[threadIdx.x] += s_sum[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) library[cell] = __logf(s_sum[0]);
}
extern "C" int spv_prepare_log1p_split(const spv_counts* x, int32_t n_cells, int32_t G, uint16_t* xb, int64_t ld_xb, float* library, void* stream) {
  if (!x || !x->X || !xb || !library || n_cells <= 0 || G <= 0 || ld_xb < 2 * (((long)G + 31) & ~31L) || (ld_xb % 128)) return fail(SPV_ERR_ARG, "spv_prepare_log1p_split: bad arguments (ld_xb a multiple of 128 words, >= 2 round_up(G, 32))%s");
  if (x->dtype != SPV_COUNT_U16 && x->dtype != SPV_COUNT_F32) return fail(SPV_ERR_ARG, "spv_prepare_log1p_split: unknown count dtype%s");
  hipLaunchKernelGGL(prepare_log1p_split_kernel, dim3((unsigned)n_cells), dim3(256), 0, (hipStream_t)stream, x->X, (long)x->ld, x->col_off,
                     (int)(x->dtype == SPV_COUNT_U16), G, (bf16_t*)xb, (long)ld_xb, library);
  return launch_status("spv_prepare_log1p_split");
}

extern "C" int spv_prepare_log1p(const spv_counts* x, int32_t n_cells, int32_t G, uint16_t* xb, int64_t ld_xb, float* library, void* stream) {
  if (!x || !x->X || !xb || !library || n_cells <= 0 || G <= 0 || ld_xb < G) return fail(SPV_ERR_ARG, "spv_prepare_log1p: bad arguments%s");
  if (x->dtype != SPV_COUNT_U16 && x->dtype != SPV_COUNT_F32) return fail(SPV_ERR_ARG, "spv_prepare_log1p: unknown count dtype%s");
  hipLaunchKernelGGL(prepare_log1p_kernel, dim3((unsigned)n_cells), dim3(256), 0, (hipStream_t)stream, x->X, (long)x->ld, x->col_off,
                     (int)(x->dtype == SPV_COUNT_U16), G, xb, (long)ld_xb, library);
  return launch_status("spv_prepare_log1p");
}


// ---------------------------------------------------------------------------------------------
// CSR-resident counts: the minibatch's rows densified into [B][ldx] (+ the log1p image of spv_prepare_log1p or
// spv_prepare_log1p_split, + the library) -- exactly the bytes the dense-resident path feeds the downstream kernels, which then run
// on the minibatch buffers with identity rows.  One workgroup per minibatch row, every group of the call in one grid
// (blockIdx.y = group).  A row is walked in windows of CSR_WIN genes (a multiple of 256): the row's stored entries whose columns fall
// in the window are scattered into a zeroed fp32 LDS image, every output is then stored 8
// genes (16 B) per lane, and a separate LDS-only pass adds log1p(x) per thread with stride 256 in increasing gene order -- the
// accumulation order of prepare_log1p_kernel (absent genes add +0.0 there, which changes no sum) -- followed by the same 256 -> 1 tree.
// ---------------------------------------------------------------------------------------------
#define CSR_WIN 8192
struct CsrGatherBatch { spv_csr_gather_args p[SPV_CSR_GATHER_MAXG]; };

__global__ __launch_bounds__(256) void csr_gather_kernel(CsrGatherBatch a) {
#pragma clang fp contract(off)   // acc += log1p(x) must stay a multiply then an add, as in prepare_log1p_kernel (no fused v_fmac)
  __shared__ __attribute__((aligned(16))) float s_c[CSR_WIN];
  __shared__ float s_sum[256];
  const spv_csr_gather_args& q = a.p[blockIdx.y];
  const int b = blockIdx.x;
  if (b >= q.B) return;   // (uniform per workgroup)
  const int t = threadIdx.x;
  const int r = q.rows[b];
  long p = 0, end = 0;
  if (r >= 0 && r < q.n_rows) { p = q.indptr[r]; end = q.indptr[r + 1]; }   // (a row outside the matrix reads as empty)
  const bool u16 = q.dtype == SPV_COUNT_U16;
  const bool split = q.xb_split != 0;
  const long ld_img = q.xb ? (split ? q.ld_xb / 2 : q.ld_xb) : 0;   // genes per image row (split: hi words)
  const long ext = q.ldx > ld_img ? q.ldx : ld_img;
  const int G = q.G;
  float acc = 0.f;
  for (long w0 = 0; w0 < ext; w0 += CSR_WIN) {
    const int wn = (int)(((long)G - w0) < CSR_WIN ? ((long)G - w0) : CSR_WIN);   // genes of the group in this window (<= 0: padding only)
    if (wn > 0) {
      for (int i = 4 * t; i < wn; i += 1024) *reinterpret_cast<f4v*>(s_c + i) = f4v{0.f, 0.f, 0.f, 0.f};
      __syncthreads();
      // every window filters the row's entries by column (a row's columns are a few KB; a binary search for the window's range
      // would put a chain of dependent global loads in front of every window)
      for (long i = p + t; i < end; i += 256) {
        const int c = q.cols[i] - (int)w0;
        if ((unsigned)c < (unsigned)wn)
          s_c[c] = u16 ? (float)reinterpret_cast<const unsigned short*>(q.vals)[i] : reinterpret_cast<const float*>(q.vals)[i];
      }
      __syncthreads();
    }
    const long wend = (w0 + CSR_WIN) < ext ? (w0 + CSR_WIN) : ext;
    for (long g = w0 + 8 * t; g < wend; g += 2048) {
      float c[8];
      if (g + 8 <= G) {
        const f4v c0 = *reinterpret_cast<const f4v*>(s_c + (g - w0)), c1 = *reinterpret_cast<const f4v*>(s_c + (g - w0) + 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) { c[j] = c0[j]; c[4 + j] = c1[j]; }
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) c[j] = (g + j < G) ? s_c[g + j - w0] : 0.f;
      }
      if (g < q.ldx) {
        if (u16) {
          u4v w;
#pragma unroll
          for (int j = 0; j < 4; ++j) w[j] = (unsigned)c[2 * j] | ((unsigned)c[2 * j + 1] << 16);
          *reinterpret_cast<u4v*>(reinterpret_cast<unsigned short*>(q.X) + (long)b * q.ldx + g) = w;
        } else {
          float* dst = reinterpret_cast<float*>(q.X) + (long)b * q.ldx + g;
          *reinterpret_cast<f4v*>(dst) = f4v{c[0], c[1], c[2], c[3]};
          *reinterpret_cast<f4v*>(dst + 4) = f4v{c[4], c[5], c[6], c[7]};
        }
      }
      if (g < ld_img) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (g + j < G) ? log1p_count(c[j]) : 0.f;
        if (!split) {
          u4v w;
#pragma unroll
          for (int j = 0; j < 4; ++j) w[j] = (unsigned)f2h(v[2 * j]) | ((unsigned)f2h(v[2 * j + 1]) << 16);
          *reinterpret_cast<u4v*>(q.xb + (long)b * q.ld_xb + g) = w;
        } else {
          u4v wh, wl;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const bf16_t h0 = f2bf(v[2 * j]), h1 = f2bf(v[2 * j + 1]);
            wh[j] = (unsigned)h0 | ((unsigned)h1 << 16);
            wl[j] = (unsigned)f2bf(v[2 * j] - bf2f(h0)) | ((unsigned)f2bf(v[2 * j + 1] - bf2f(h1)) << 16);
          }
          const long o = (long)b * q.ld_xb + (g >> 5) * 64 + (g & 31);
          *reinterpret_cast<u4v*>(q.xb + o) = wh;
          *reinterpret_cast<u4v*>(q.xb + o + 32) = wl;
        }
      }
    }
    if (q.library)   // the dense kernel's order: this thread's genes t, t + 256, ... (windows start at multiples of 256)
      for (int i = t; i < wn; i += 256) acc += log1p_count(s_c[i]);
    __syncthreads();   // (the next window re-zeroes s_c)
  }
  if (!q.library) return;
  s_sum[t] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) s_sum[t] += s_sum[t + o];
    __syncthreads();
  }
  if (t == 0) q.library[b] = __logf(s_sum[0]);
}

extern "C" int spv_csr_gather(const spv_csr_gather_args* groups, int32_t n_groups, void* stream) {
  if (!groups || n_groups <= 0 || n_groups > SPV_CSR_GATHER_MAXG) return fail(SPV_ERR_ARG, "spv_csr_gather: bad group count%s");
  CsrGatherBatch a{};
  int bmax = 0;
  for (int i = 0; i < n_groups; ++i) {
    const spv_csr_gather_args& q = groups[i];
    if (!q.indptr || !q.cols || !q.vals || !q.rows || !q.X) return fail(SPV_ERR_ARG, "spv_csr_gather: null pointer%s");
    if (q.n_rows <= 0 || q.G <= 0 || q.B <= 0) return fail(SPV_ERR_ARG, "spv_csr_gather: n_rows, G and B must be positive%s");
    if (q.dtype != SPV_COUNT_U16 && q.dtype != SPV_COUNT_F32) return fail(SPV_ERR_ARG, "spv_csr_gather: unknown count dtype%s");
    if (q.ldx < q.G || (q.ldx % 8) || (reinterpret_cast<uintptr_t>(q.X) & 15))
      return fail(SPV_ERR_ARG, "spv_csr_gather: X needs ldx >= G, ldx a multiple of 8 and a 16-byte aligned base%s");
    if (q.xb) {
      if (!q.library) return fail(SPV_ERR_ARG, "spv_csr_gather: an image needs the library%s");
      if (reinterpret_cast<uintptr_t>(q.xb) & 15) return fail(SPV_ERR_ARG, "spv_csr_gather: xb needs a 16-byte aligned base%s");
      if (q.xb_split ? (q.ld_xb < 2 * (((long)q.G + 31) & ~31L) || (q.ld_xb % 128)) : (q.ld_xb < q.G || (q.ld_xb % 8)))
        return fail(SPV_ERR_ARG, "spv_csr_gather: ld_xb breaks the image layout (f16: >= G, a multiple of 8; split: a multiple of 128, >= 2 round_up(G, 32))%s");
    }
    a.p[i] = q;
    bmax = q.B > bmax ? q.B : bmax;
  }
  hipLaunchKernelGGL(csr_gather_kernel, dim3((unsigned)bmax, (unsigned)n_groups), dim3(256), 0, (hipStream_t)stream, a);
  return launch_status("spv_csr_gather");
}
